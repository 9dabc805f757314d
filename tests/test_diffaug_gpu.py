"""GPU: the opt-in differentiable augmentation of the discriminator's inputs (--D_aug) on the HIP path, against the
CPU restatement composed with the oracle (tests/diffaug_cases.py) —
  (1) the two grouped kernels: translation / cutout bit-exact, colour against float64 at a derived bound, the refusals;
  (2) three training iterations against the oracle loop, graph replay against eager;
  (3) off means off, and the launch budget with the policy on;
  (4) the gradient reaches the generator through the augmentation;
  (5) the command line: checkpoints and sampling are untouched."""
import ctypes
import glob
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import diffaug_cases as DA
import schedule_cases as S
from oracle import tganv2_oracle as O
from txt2vid_amd import functional_aug as A

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
V, B = S.V, S.B

# name -> (shapes of the member tensors, row strides, rows of the parameter block)
SHAPES = {
    'bench_b32': ([(32, 1, 16, 8, 8), (16, 1, 8, 16, 16), (8, 1, 4, 32, 32), (4, 1, 2, 64, 64)], [1, 2, 4, 8], 32),
    'rgb128_b16': ([(16, 3, 16, 16, 16), (8, 3, 8, 32, 32), (4, 3, 4, 64, 64), (2, 3, 2, 128, 128)], [1, 2, 4, 8], 16),
    'single_level': ([(4, 1, 16, 64, 64)], [1], 4),
    'odd_batch': ([(5, 1, 8, 8, 8), (3, 1, 4, 16, 16), (2, 1, 2, 32, 32), (1, 1, 1, 64, 64)], [1, 2, 4, 8], 5),
}


def seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def _inputs(name, s=0):
    shapes, strides, rows = SHAPES[name]
    g = torch.Generator()
    g.manual_seed(1234 + s)
    xs = [torch.rand(*sh, generator=g) * 2 - 1 for sh in shapes]
    gys = [torch.randn(*sh, generator=g) for sh in shapes]
    u = torch.rand(rows, A.K, generator=g)
    return xs, gys, u, strides


def _device_run(xs, gys, u, strides, policy, needs=None):
    """Forward + backward through the kernels. Returns (ys, gxs) on the host (gxs[i] None where member i needs no gradient)."""
    needs = [True] * len(xs) if needs is None else needs
    xd = [x.to(DEV).requires_grad_(n) for x, n in zip(xs, needs)]
    ud = u.to(DEV)
    ys = A.diffaug(xd, [ud] * len(xd), strides, policy)
    live = [i for i, n in enumerate(needs) if n]
    grads = torch.autograd.grad([ys[i] for i in live], [xd[i] for i in live], [gys[i].to(DEV) for i in live]) if live else ()
    gxs = [None] * len(xs)
    for i, gr in zip(live, grads):
        gxs[i] = gr.cpu()
    return [y.detach().cpu() for y in ys], gxs, ys


def _cpu_run(xs, gys, u, strides, policy, dtype):
    ys, gxs = [], []
    for x, gy, st in zip(xs, gys, strides):
        xr = x.to(dtype).requires_grad_(True)
        y = DA.augment(xr, u, policy, st)
        gx, = torch.autograd.grad(y, xr, gy.to(dtype))
        ys.append(y.detach())
        gxs.append(gx)
    return ys, gxs


# ------------------------------------------------------------------------------------------------ 1. op level
@pytest.mark.parametrize('name', sorted(SHAPES))
@pytest.mark.parametrize('policy', ['translation', 'cutout', 'translation,cutout'])
def test_gathers_and_masks_are_bit_exact(name, policy):
    """translation, cutout and their combination are pure gathers and masks: forward and backward equal the fp32 restatement
    bit for bit (every member of a pyramid in ONE launch per direction)."""
    xs, gys, u, strides = _inputs(name)
    ys, gxs, _ = _device_run(xs, gys, u, strides, policy)
    want_y, want_g = _cpu_run(xs, gys, u, strides, policy, torch.float32)
    for i in range(len(xs)):
        assert torch.equal(ys[i], want_y[i]), (name, policy, i)
        assert torch.equal(gxs[i], want_g[i]), (name, policy, i)
        assert not torch.equal(ys[i], xs[i])


def _colour_bounds(C, n, X, G):
    """See test_colour_against_float64."""
    red = 0.5 * (-(-n // 256) + 11)
    return EPS * X * (36 * (C + 10) + red), EPS * G * (12 * (C + 8) + 3 * red)


@pytest.mark.parametrize('name', sorted(SHAPES))
@pytest.mark.parametrize('policy', ['color', 'color,translation', 'color,cutout', DA.FULL])
def test_colour_against_float64(name, policy):
    """The colour map against the float64 restatement. Bound (derived from the fp32 operation count and the reduction length, with
    eps = 2^-24, X = max(1, max|x|), G = max|dL/dy|, n = elements of a clip, C = channels):

    forward, per element: b and c carry one rounding each; the channel mean C - 1 additions and a multiplication by a rounded
    1 / C; x - m, m + b, the saturation FMA, t - mu and the contrast FMA one each: at most C + 10 roundings. No intermediate
    exceeds 12 X (|t| <= 2 * 2 X + X + 0.5, |y| <= 1.5 * (|t| + |mu|) + |mu|), and an error made before the last step is
    amplified by at most s * c <= 3: 36 (C + 10) eps X. The clip mean: a thread adds at most ceil(n / 256) terms in sequence,
    then 6 shuffle steps, 3 additions across the waves, the division and + b: its error is at most (ceil(n / 256) + 11) eps X,
    and it enters y through (1 - c) mu, |1 - c| <= 0.5.
        |dy| <= eps X (36 (C + 10) + 0.5 (ceil(n / 256) + 11))
    backward: at most C + 8 roundings per element, no intermediate above 6 G (|g2| <= 2 G, |s g2 + (1 - s) pm| <= 6 G), amplified
    by at most s <= 2: 12 (C + 8) eps G; the mean of the gradient as above with G, entering through (1 - c) <= 0.5 and then
    s + |1 - s| <= 3.
        |dgx| <= eps G (12 (C + 8) + 1.5 (ceil(n / 256) + 11))
    where translation / cutout only select which elements enter."""
    xs, gys, u, strides = _inputs(name, 1)
    ys, gxs, _ = _device_run(xs, gys, u, strides, policy)
    want_y, want_g = _cpu_run(xs, gys, u, strides, policy, torch.float64)
    for i, x in enumerate(xs):
        C, n = x.shape[1], x[0].numel()
        by, bg = _colour_bounds(C, n, max(1.0, float(x.abs().max())), float(gys[i].abs().max()))
        ey = float((ys[i].double() - want_y[i]).abs().max())
        eg = float((gxs[i].double() - want_g[i]).abs().max())
        print('%s %s member %d (C=%d, n=%d): forward measured/bound = %.3e / %.3e = %.4f, backward %.3e / %.3e = %.4f'
              % (name, policy, i, C, n, ey, by, ey / by, eg, bg, eg / bg))
        assert ey <= by, (name, policy, i, ey, by)
        assert eg <= bg, (name, policy, i, eg, bg)
    # a second run gives the same bits (fixed-order reduction; every workgroup of a split clip computes the same mean)
    ys2, _, _ = _device_run(xs, gys, u, strides, policy)
    assert all(torch.equal(a, b) for a, b in zip(ys, ys2))


def _counted(run, names=('t2v_diffaug_fwd', 't2v_diffaug_bwd')):
    """Run `run()` with counting wrappers around the entry points of the loaded library; also records the member counts."""
    from txt2vid_amd import functional as TF
    l = TF.lib()
    orig = {n: getattr(l, n) for n in names}
    calls = {n: 0 for n in names}
    members = {n: [] for n in names}

    def wrap(n):
        def f(*a):
            calls[n] += 1
            members[n].append(a[1])
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


def test_member_without_grad_gets_no_backward_work():
    xs, gys, u, strides = _inputs('bench_b32', 2)
    needs = [False, True, False, True]
    calls, members, (ys, gxs, dev_ys) = _counted(lambda: _device_run(xs, gys, u, strides, DA.FULL, needs))
    assert calls == {'t2v_diffaug_fwd': 1, 't2v_diffaug_bwd': 1}
    assert members == {'t2v_diffaug_fwd': [4], 't2v_diffaug_bwd': [2]}
    assert [y.requires_grad for y in dev_ys] == needs
    want_y, want_g = _cpu_run(xs, gys, u, strides, DA.FULL, torch.float64)
    for i, x in enumerate(xs):
        by, bg = _colour_bounds(1, x[0].numel(), 1.0, float(gys[i].abs().max()))
        assert float((ys[i].double() - want_y[i]).abs().max()) <= by
        if needs[i]:
            assert float((gxs[i].double() - want_g[i]).abs().max()) <= bg
        else:
            assert gxs[i] is None
    # nothing requires a gradient (the D step's detached clips): no backward at all, plain outputs
    calls, _, (_, _, dev_ys) = _counted(lambda: _device_run(xs, gys, u, strides, DA.FULL, [False] * 4))
    assert calls == {'t2v_diffaug_fwd': 1, 't2v_diffaug_bwd': 0} and not any(y.requires_grad for y in dev_ys)


@pytest.mark.parametrize('S_', [16, 64])
def test_parameter_extremes(S_):
    """tx, ty at both ends of their range; a cutout wholly inside the frame and one clipped by the border (rows 0 / 1: centre in
    the middle, rows 2 / 3: centre at the first and at the last position)."""
    top = float(np.nextafter(np.float32(1), np.float32(0)))
    u = torch.full((4, A.K), 0.5)
    u[0, 3], u[0, 4] = 0.0, top
    u[1, 3], u[1, 4] = top, 0.0
    u[2, 5], u[2, 6] = 0.0, 0.0
    u[3, 5], u[3, 6] = top, 0.0
    g = torch.Generator()
    g.manual_seed(S_)
    x = torch.rand(4, 2, 3, S_, S_, generator=g) * 2 - 1
    gy = torch.randn(4, 2, 3, S_, S_, generator=g)
    P = A.aug_params(u, S_)
    r, size = P['r'], P['size']
    assert P['tx'].tolist() == [-r, r, 0, 0] and P['ty'].tolist() == [r, -r, 0, 0]
    assert P['x0'].tolist()[2:] == [-(size // 2), S_ - size // 2] and P['x0'].tolist()[0] == S_ // 2 - size // 2
    (y,), (gx,), _ = _device_run([x], [gy], u, [1], 'translation,cutout')
    (wy,), (wg,) = _cpu_run([x], [gy], u, [1], 'translation,cutout', torch.float32)
    assert torch.equal(y, wy) and torch.equal(gx, wg)
    (yt,), _, _ = _device_run([x], [gy], u, [1], 'translation')
    assert torch.equal(yt[0, :, :, r:, :S_ - r], x[0, :, :, :S_ - r, r:]) and float(yt[0, :, :, :r].abs().sum()) == 0
    assert torch.equal(yt[1, :, :, :S_ - r, r:], x[1, :, :, r:, :S_ - r]) and float(yt[1, :, :, :, :r].abs().sum()) == 0
    (yc,), _, _ = _device_run([x], [gy], u, [1], 'cutout')
    lo = S_ // 2 - size // 2
    assert float(yc[0, :, :, lo:lo + size, lo:lo + size].abs().sum()) == 0                  # wholly inside
    assert int((yc[0] == 0).sum()) == 2 * 3 * size * size
    assert float(yc[2, :, :, :size - size // 2, :size - size // 2].abs().sum()) == 0       # clipped at the top-left corner
    assert int((yc[2] == 0).sum()) == 2 * 3 * (size - size // 2) ** 2
    assert float(yc[3, :, :, :size - size // 2, S_ - size // 2:].abs().sum()) == 0         # clipped at the top-right corner
    assert int((yc[3] == 0).sum()) == 2 * 3 * (size - size // 2) * (size // 2)


def test_entry_points_refuse_bad_arguments():
    from txt2vid_amd import functional as TF
    from txt2vid_amd._lib import AugMember, MAX_GROUPS
    l, st = TF.lib(), TF._stream()
    x = torch.ones(2, 1, 2, 8, 8, device=DEV)
    y = torch.full_like(x, 7.0)
    u = torch.rand(2, A.K, device=DEV)

    def member(**kw):
        m = dict(x=x.data_ptr(), y=y.data_ptr(), u=u.data_ptr(), N=2, C=1, T=2, S=8, row_stride=1, rows=2, policy=7)
        m.update(kw)
        return m

    def call(fn, ms, n=None):
        arr = (AugMember * max(1, len(ms)))()
        for a, m in zip(arr, ms):
            for k, v in m.items():
                setattr(a, k, v)
        return fn(arr, len(ms) if n is None else n, st)
    for fn in (l.t2v_diffaug_fwd, l.t2v_diffaug_bwd):
        assert fn(None, 1, st) < 0
        assert call(fn, [member()], n=0) < 0
        assert call(fn, [member()] * (MAX_GROUPS + 1)) < 0                       # more than MAX_GROUPS members
        for bad in (dict(policy=8), dict(policy=15), dict(policy=0), dict(policy=-1), dict(x=None), dict(y=None), dict(u=None),
                    dict(y=x.data_ptr()), dict(N=0), dict(C=0), dict(T=0), dict(S=0), dict(row_stride=0), dict(rows=1),
                    dict(row_stride=2)):
            assert call(fn, [member(), member(**bad)]) < 0, bad
    torch.cuda.synchronize()
    assert bool((y == 7).all())                                                   # nothing was launched
    assert call(l.t2v_diffaug_fwd, [member()]) == 0
    torch.cuda.synchronize()
    assert not bool((y == 7).any())
    with pytest.raises(ValueError):
        A.diffaug([x] * 9, [u] * 9, [1] * 9, 7)
    with pytest.raises(RuntimeError):
        A.diffaug([x.cpu()], [u], [1], 7)                                         # no CPU fallback
    with pytest.raises(ValueError):
        A.diffaug([x], [u], [1], 'colour')


# ------------------------------------------------------------------------------------------------ helpers for the runs
def pour(module):
    module.load_state_dict({k: O.recipe_tensor(k, v.shape) for k, v in module.state_dict().items()})
    return module.to(DEV)


def tokens_for(batch, s=77):
    tg = torch.Generator()
    tg.manual_seed(s)
    t = torch.randint(4, V, (batch, 8), generator=tg)
    t[:, 0], t[:, -1] = 1, 2
    return t


NO_ATTR = object()


def make(cond=False, N=1, M=1, policy=DA.FULL):
    """The B = 4, 64x64x1 set-up of the step tests (recipe weights, RSGAN + GP 0.5, Adam). `policy=NO_ATTR`: a parameter object
    without the D_aug attribute at all."""
    from txt2vid_amd.gan.cond_gan import CondGan
    from txt2vid_amd.gan.losses import MixedGanLoss, RSGANLoss
    from txt2vid_amd.optim import Adam
    txt = None
    if cond:
        from txt2vid_amd.models.tganv2_cond.gen import MultiScaleGen
        from txt2vid_amd.models.tganv2_cond.discrim import MultiScaleDiscrim
        from txt2vid_amd.models.txt.basic import Seq2Seq
        gen = pour(MultiScaleGen(width=64, height=64, num_channels=1, cond_dim=256)).train()
        dis = pour(MultiScaleDiscrim(num_channels=1, cond_dim=256)).train()
        txt = Seq2Seq(vocab_size=V)
        txt.load_state_dict({k: O.recipe_tensor(k if k.startswith('encoder.') else 'encoder.' + k[len('decoder.'):], v.shape)
                             for k, v in txt.state_dict().items()})
        txt.to(DEV)
    else:
        from txt2vid_amd.models.tganv2.gen import MultiScaleGen
        from txt2vid_amd.models.tganv2.discrim import MultiScaleDiscrim
        gen = pour(MultiScaleGen(width=64, height=64, num_channels=1)).train()
        dis = pour(MultiScaleDiscrim(num_channels=1)).train()
    gan = CondGan(gen=gen, discrims=[dis], cond_encoder=txt, discrim_names=['video'])
    optD = Adam([{'params': dis.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    optG = Adam([{'params': gen.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    prm = S.params_for(dict(N=N, M=M, gp=0.5, mean_d=False, mean_g=False))
    if policy is not NO_ATTR:
        prm.D_aug = policy
    return gan, optD, optG, MixedGanLoss(g_loss=RSGANLoss(), d_loss=RSGANLoss()), prm


def batches(n=4, s=12):
    g = torch.Generator()
    g.manual_seed(s)
    return [(torch.rand(B, 1, 16, 64, 64, generator=g) * 2 - 1).to(DEV) for _ in range(n)]


# ------------------------------------------------------------------------------------------------ 2. iteration level
@pytest.mark.parametrize('cond', [False, True])
@pytest.mark.parametrize('N,M', [(1, 1), (2, 1)])
def test_iterations_vs_oracle_loop(cond, N, M):
    """Three iterations with the full policy against the oracle loop with the restatement at the same call sites and draw
    positions: lossD and lossG at the bounds of the conditioning-augmentation loop test (1e-3, then 2e-2 in the third iteration:
    the GAN dynamics are chaotic)."""
    from txt2vid_amd.gan.trainer import TrainStep
    tokens = tokens_for(B) if cond else None
    ref = DA.oracle_loop(cond, N, M, DA.FULL, tokens=tokens, iters=3)
    gan, optD, optG, losses, prm = make(cond, N, M)
    seed(100)
    for it in range(3):
        x = S.batch().to(DEV)
        c = None
        if cond:
            with torch.no_grad():
                c = gan.cond_encoder.encode(tokens.to(DEV), [8] * B)[2].detach()
        ts = TrainStep(gan, optD, optG, losses, prm, DEV)
        assert ts.aug == 7
        lD, lG, _, _ = ts.run(x, c)
        lD, lG = float(lD), float(lG)
        tol = 1e-3 if it < 2 else 2e-2
        print('D_aug %s %d:%d it %d: lossD %.6f (%.6f) lossG %.6f (%.6f)' % ('cond' if cond else 'uncond', N, M, it, lD,
                                                                             ref['lossD'][it], lG, ref['lossG'][it]))
        assert abs(lD - ref['lossD'][it]) < tol * max(1.0, abs(ref['lossD'][it]))
        assert abs(lG - ref['lossG'][it]) < tol * max(1.0, abs(ref['lossG'][it]))


def test_graph_replay_matches_eager():
    """GraphedTrainStep with the full policy (the blocks among the device-resident draws, the launches inside the one captured
    graph) reproduces the eager iterations: 2 eager, then capture + replays. Tolerances of test_ca_graph_replay_matches_eager."""
    from txt2vid_amd.gan.trainer import TrainStep, GraphedTrainStep
    gan, optD, optG, losses, prm = make(N=1, M=2)
    seed(6)
    eager = []
    for x in batches():
        lD, lG, _, _ = TrainStep(gan, optD, optG, losses, prm, DEV).run(x, None)
        eager.append((float(lD), float(lG)))
    gan, optD, optG, losses, prm = make(N=1, M=2)
    seed(6)
    gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (B, 1, 16, 64, 64), warmup=2)
    assert gs.draws.n_aug == 2 * 1 + 2 + 1
    for i, x in enumerate(batches()):
        lD, lG = gs.step(x)
        got = (float(lD), float(lG))
        print('D_aug step %d (%s): %s vs eager %s' % (i, 'replay' if i >= 2 else 'eager', got, eager[i]))
        tol = 2e-5 if i < 2 else 2e-3
        assert all(abs(a - b) < tol for a, b in zip(got, eager[i])), (i, got, eager[i])
    assert gs.graphs is not None and gs.n_graphs == 1


# ------------------------------------------------------------------------------------------------ 3. off means off
def _one_eager_iteration(parts):
    from txt2vid_amd.gan.trainer import TrainStep
    gan, optD, optG, losses, prm = parts
    seed(100)
    lD, lG, _, _ = TrainStep(gan, optD, optG, losses, prm, DEV).run(batches(1)[0], None)
    return float(lD), float(lG)


def _three_graphed_iterations(parts):
    from txt2vid_amd.gan.trainer import GraphedTrainStep
    gan, optD, optG, losses, prm = parts
    seed(100)
    gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (B, 1, 16, 64, 64), warmup=2)
    out = []
    for x in batches(3):
        lD, lG = gs.step(x)
        out.append((float(lD), float(lG)))
    assert gs.graphs is not None
    return out


def test_off_means_off():
    """With the flag absent (no attribute at all) or empty, no call of the new entry points is made, eagerly or while capturing,
    and a step's losses are bit-identical between the two."""
    _one_eager_iteration(make(policy=NO_ATTR))                                       # burn-in
    calls, _, plain = _counted(lambda: _one_eager_iteration(make(policy=NO_ATTR)))
    assert calls == {'t2v_diffaug_fwd': 0, 't2v_diffaug_bwd': 0}
    calls, _, off = _counted(lambda: _one_eager_iteration(make(policy='')))
    assert calls == {'t2v_diffaug_fwd': 0, 't2v_diffaug_bwd': 0}
    print('flag empty %r | no attribute %r' % (off, plain))
    assert off == plain
    calls, _, _ = _counted(lambda: _three_graphed_iterations(make(policy='')))
    assert calls == {'t2v_diffaug_fwd': 0, 't2v_diffaug_bwd': 0}
    calls, _, on = _counted(lambda: _one_eager_iteration(make()))
    assert on != plain and all(np.isfinite(on))


@pytest.mark.parametrize('N,M', [(1, 1), (2, 2)])
def test_launch_budget(N, M):
    """Full policy, 4 levels, the fused paths: one forward launch per D step and per G step (real + generated pyramid = 8 members;
    a later G step augments the generated pyramid only) and one backward launch per G step over the 4 generated members. Nowhere
    a second launch for the reduction. Counted per Python pass: one eager iteration, and the 2 eager + 1 captured pass of a
    graphed run (the replay itself makes no call)."""
    calls, members, _ = _counted(lambda: _one_eager_iteration(make(N=N, M=M)))
    assert calls == {'t2v_diffaug_fwd': N + M, 't2v_diffaug_bwd': M}
    assert members['t2v_diffaug_fwd'] == [8] * (N + 1) + [4] * (M - 1)
    assert members['t2v_diffaug_bwd'] == [4] * M
    calls, _, _ = _counted(lambda: _three_graphed_iterations(make(N=N, M=M)))
    assert calls == {'t2v_diffaug_fwd': 3 * (N + M), 't2v_diffaug_bwd': 3 * M}


# ------------------------------------------------------------------------------------------------ 4. gradient reaches G
def test_gradient_reaches_the_generator():
    """The generator's gradient flows back through the augmentation: finite, and different from the policy-off gradient. With
    cutout alone, the gradient arriving at every rendered level is exactly 0 inside the cut box and exactly the upstream
    gradient outside it."""
    from txt2vid_amd.models.tganv2.gen import MultiScaleGen
    gen = pour(MultiScaleGen(width=64, height=64, num_channels=1)).train()
    g = torch.Generator()
    g.manual_seed(9)
    z = torch.randn(B, 256, generator=g).to(DEV)
    u = torch.rand(B, A.K, generator=g)
    ws = None
    grads = {}
    for policy in ('', DA.FULL, 'cutout'):
        gen.zero_grad()
        seed(5)
        fake = gen(z)
        if ws is None:
            ws = [torch.randn(*f.shape, generator=g) + 3.0 for f in fake]            # (no zero among the upstream gradients)
        for f in fake:
            f.retain_grad()
        out = A.diffaug(fake, [u.to(DEV)] * len(fake), [2 ** l for l in range(len(fake))], policy)
        loss = sum((o * w.to(DEV)).sum() for o, w in zip(out, ws))
        loss.backward()
        grads[policy] = gen.fc.weight.grad.detach().clone()
        assert bool(torch.isfinite(grads[policy]).all())
        if policy == 'cutout':
            for l, (f, w) in enumerate(zip(fake, ws)):
                Sd = f.shape[-1]
                P = A.aug_params(u, Sd)
                for j in range(f.shape[0]):
                    r = j * 2 ** l
                    x0, y0, size = int(P['x0'][r]), int(P['y0'][r]), P['size']
                    idx = torch.arange(Sd)
                    cut = ((idx >= y0) & (idx < y0 + size))[:, None] & ((idx >= x0) & (idx < x0 + size))[None, :]
                    gj = f.grad[j].cpu()
                    assert int(cut.sum()) > 0
                    assert float(gj[:, :, cut].abs().max()) == 0.0
                    assert torch.equal(gj[:, :, ~cut], w[j][:, :, ~cut])
    assert not torch.equal(grads[DA.FULL], grads[''])
    assert not torch.equal(grads['cutout'], grads[''])
    rel = float((grads[DA.FULL] - grads['']).norm() / grads[''].norm())
    print('fc.weight gradient, full policy vs off: relative difference %.3e' % rel)
    assert rel > 1e-3


# ------------------------------------------------------------------------------------------------ 5. command line
def _cli(args, timeout=600):
    p = subprocess.run([sys.executable, '-m', 'txt2vid_amd.train.gan'] + args, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=timeout)
    out = p.stdout.decode(errors='replace')
    assert p.returncode == 0, out[-3000:]
    return out


def test_cli_train_checkpoint_and_sampling(tmp_path):
    base = ['--data', os.path.join(ROOT, 'tools', 'cfg', 'synth.json'), '--num_channels', '1', '--cuda', '--frame_sizes', '8', '16',
            '32', '64', '--D_names', 'video', '--G_lr', '0.0002', '--D_lr', '0.0002', '--D_beta1', '0.5', '--D_beta2', '.999',
            '--G_beta1', '0.5', '--G_beta2', '.999', '--D_loss', 'txt2vid.gan.losses.RSGANLoss', '--init_method', 'xavier',
            '--seed', '100', '--gp_lambda', '.5', '--subsample_input', '--workers', '0', '--log_period', '1',
            '--G', 'txt2vid.models.tganv2.gen.MultiScaleGen', '--D', 'txt2vid.models.tganv2.discrim.MultiScaleDiscrim',
            '--dont_use_sent', '--batch_size', '8', '--epochs', '1']

    def train(name, extra):
        out = str(tmp_path / name)
        log = _cli(base + ['--out', out, '--out_samples', str(tmp_path / (name + '_s')), '--max_iters', '3', '--save_model_period', '3',
                           '--save_example_period', '0'] + extra)
        assert 'Iter 3, Loss_D' in log
        ck = glob.glob(os.path.join(out, 'iter_3_lossG_*'))
        assert len(ck) == 1
        return ck[0], log
    ck_on, log_on = train('on', ['--D_aug', DA.FULL])
    assert 'HIP-graph replay' in log_on
    ck_eager, log_eager = train('eager', ['--D_aug', DA.FULL, '--no_graph'])
    assert 'HIP-graph replay' not in log_eager
    ck_off, _ = train('off', [])

    def keys(path):
        sd = torch.load(path, map_location='cpu', weights_only=False)
        return {k: (sorted(v.keys()) if isinstance(v, dict) else None) for k, v in sd.items()}
    assert keys(ck_on) == keys(ck_off) == keys(ck_eager)
    a = torch.load(ck_on, map_location='cpu', weights_only=False)['gen']
    b = torch.load(ck_off, map_location='cpu', weights_only=False)['gen']
    assert not torch.equal(a['fc.weight'], b['fc.weight'])                          # the flag did change the training
    # the checkpoint of the run with the flag loads into a run without it
    log = _cli(base + ['--out', str(tmp_path / 'resume'), '--out_samples', str(tmp_path / 'resume_s'), '--weights', ck_on,
                       '--max_iters', '2', '--save_model_period', '1000', '--save_example_period', '0'])
    assert 'Iter 2, Loss_D' in log
    # sampling never augments: the same files with and without the flag
    files = {}
    for name, extra in (('t_on', ['--D_aug', DA.FULL]), ('t_off', [])):
        smp = str(tmp_path / name)
        _cli(base + ['--out', str(tmp_path / 'resume'), '--out_samples', smp, '--test', '--weights', ck_on, '--num_samples', '1',
                     '--max_iters', '1'] + extra)
        files[name] = {os.path.basename(f): open(f, 'rb').read() for f in sorted(glob.glob(os.path.join(smp, '*')))}
        assert 'real_0.png' in files[name] and '64x64_0_0.jpg' in files[name]
    assert files['t_on'] == files['t_off']
    # an unknown name is refused by the parser
    p = subprocess.run([sys.executable, '-m', 'txt2vid_amd.train.gan'] + base + ['--D_aug', 'colour'], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 2 and b'--D_aug' in p.stdout
