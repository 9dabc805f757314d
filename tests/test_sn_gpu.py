"""GPU: the opt-in spectral normalisation of the discriminator (--D_sn) —
  (1) the two entry points, phase by phase, against float64 on the kernel's own fp32 inputs at derived bounds (tests/sn_cases.py);
      alignment, many jobs, the zero matrix, repeatability, convergence;
  (2) the model: the discriminator really multiplies with W / sigma everywhere (packed copies included), graph replay against
      eager with two discriminator steps, off means off;
  (3) the command line: checkpoint state, resume, the refusal without the flag."""
import glob
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import sn_cases as S
from oracle import tganv2_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ 1. op level
def _dev(t, off=0):
    """A device copy `off` elements into a 16-byte aligned buffer (off = 1: 4 bytes off 16-byte alignment)."""
    buf = torch.empty(t.numel() + off, dtype=torch.float32, device=DEV)
    out = buf[off:].view(t.shape)
    out.copy_(t)
    assert (out.data_ptr() % 16 == 0) == (off % 4 == 0)
    return out


class Job(object):
    def __init__(self, W, u, G=None, off=0):
        self.M, self.K = W.shape
        self.w, self.u = _dev(W, off), _dev(u, off)
        self.what = _dev(torch.full_like(W, float('nan')), off)
        self.v, self.sigma = _dev(torch.zeros(self.K), off), _dev(torch.zeros(1), off)
        self.g = _dev(G, off) if G is not None else None


def _table(jobs):
    from txt2vid_amd._lib import SnJob
    arr = (SnJob * len(jobs))()
    for a, j in zip(arr, jobs):
        a.w, a.what, a.u, a.v, a.sigma = j.w.data_ptr(), j.what.data_ptr(), j.u.data_ptr(), j.v.data_ptr(), j.sigma.data_ptr()
        a.g, a.M, a.K = (j.g.data_ptr() if j.g is not None else None), j.M, j.K
    return arr


def _ws(arr, n):
    from txt2vid_amd import functional as TF
    need = TF.lib().t2v_sn_ws_floats(arr, n)
    assert need > 0
    return torch.empty(need, dtype=torch.float32, device=DEV)


def refresh(jobs, n_iter=1, from_param=0):
    from txt2vid_amd import functional as TF
    arr = _table(jobs)
    ws = _ws(arr, len(jobs))
    st = TF.lib().t2v_sn_refresh(arr, len(jobs), TF._p(ws), ws.numel(), n_iter, S.EPS, from_param, TF._stream())
    torch.cuda.synchronize()
    return st


def project(jobs, restore=0):
    from txt2vid_amd import functional as TF
    arr = _table(jobs)
    ws = _ws(arr, len(jobs))
    st = TF.lib().t2v_sn_project(arr, len(jobs), TF._p(ws), ws.numel(), restore, TF._stream())
    torch.cuda.synchronize()
    return st


def _within(name, got, ref, bound):
    err = (got.double().cpu() - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print('    %-8s max |delta| / bound = %.4f' % (name, ratio))
    assert bool((err <= bound).all()), (name, float(err.max()), float(bound.max()))


def check_refresh(job, W, u0):
    """One refresh of `job` from (W, u0), phase by phase; every phase's reference starts from the kernel's own fp32 output of
    the phase before (sn_cases: a sum of n products within g(n) sum |a||b|, a norm within (n + 2) E, one E per division)."""
    print('  refresh [%d, %d]' % (job.M, job.K))
    v, bv = S.phase_v(W, u0)
    _within('v', job.v, v, bv)
    u, bu, sigma, bs = S.phase_u_sigma(W, job.v.cpu())
    _within('u', job.u, u, bu)
    _within('sigma', job.sigma, torch.tensor([sigma], dtype=torch.float64), bs)
    ref, bw = S.phase_scale(W, float(job.sigma.item()))
    _within('What', job.what, ref, bw)
    assert torch.equal(job.w.cpu(), W)                       # the master is only read


def check_project(job, G0, What, u, v, sigma):
    print('  project [%d, %d]' % (job.M, job.K))
    ref, b = S.phase_project(G0, What, u, v, sigma)
    _within('dW', job.g, ref, b)


@pytest.mark.parametrize('shape', S.SHAPES, ids=lambda s: '%dx%d' % s)
def test_refresh_and_projection_against_float64(shape):
    M, K = shape
    W, u0, G = S.make_case(M, K, seed=100 + M + K)
    job = Job(W, u0, G)
    assert refresh([job]) == 0
    check_refresh(job, W, u0)
    What, u, v, sigma = job.what.cpu(), job.u.cpu(), job.v.cpu(), float(job.sigma.item())
    assert project([job], restore=1) == 0
    check_project(job, G, What, u, v, sigma)
    assert torch.equal(job.what.cpu(), W)                    # restore: the parameter's storage holds the master again
    # the optimiser's side: W updated in the parameter's storage, saved to the master by the refresh that follows
    W2 = (W + 0.01 * G).float()
    job.what.copy_(W2)
    u1 = job.u.cpu().clone()
    assert refresh([job], from_param=1) == 0
    check_refresh(job, W2, u1)


def test_unaligned_job_and_two_power_iterations():
    """Every buffer 4 bytes off 16-byte alignment (the scalar paths), K a multiple of 4 so that alignment alone decides, against
    float64 like the aligned jobs; then n_iter = 2 equals two calls with n_iter = 1, bit for bit."""
    W, u0, G = S.make_case(67, 1028, seed=7)
    job = Job(W, u0, G, off=1)
    assert refresh([job]) == 0
    check_refresh(job, W, u0)
    What, u, v, sigma = job.what.cpu(), job.u.cpu(), job.v.cpu(), float(job.sigma.item())
    assert project([job]) == 0
    check_project(job, G, What, u, v, sigma)
    assert torch.equal(job.what.cpu(), What)                 # no restore asked for
    # (the 16-byte paths add a row's products in another order than the scalar ones: an aligned copy of the job meets the same
    # bounds, not the same bits)
    aligned = Job(W, u0)
    assert refresh([aligned]) == 0
    check_refresh(aligned, W, u0)
    u1 = aligned.u.cpu().clone()
    assert refresh([aligned]) == 0
    check_refresh(aligned, W, u1)
    twice = Job(W, u0)
    assert refresh([twice], n_iter=2) == 0
    for a, b in ((aligned.v, twice.v), (aligned.u, twice.u), (aligned.sigma, twice.sigma), (aligned.what, twice.what)):
        assert torch.equal(a, b)


def test_all_shapes_in_one_call_and_identical_bits_on_a_second_run():
    cases = [S.make_case(M, K, seed=100 + M + K) for M, K in S.SHAPES] + [S.make_case(67, 1028, seed=7)]
    runs = []
    for _ in range(2):
        jobs = [Job(W, u0, G, off=(1 if i == len(cases) - 1 else 0)) for i, (W, u0, G) in enumerate(cases)]
        assert refresh(jobs) == 0
        state = [(j.what.cpu(), j.u.cpu(), j.v.cpu(), float(j.sigma.item())) for j in jobs]
        assert project(jobs) == 0
        runs.append((jobs, state))
    for (job, st), (W, u0, G) in zip(zip(*runs[0]), cases):
        check_refresh(job, W, u0)
        check_project(job, G, *st)
    for a, b in zip(runs[0][0], runs[1][0]):
        for name in ('what', 'u', 'v', 'sigma', 'g'):
            assert torch.equal(getattr(a, name), getattr(b, name)), (a.M, a.K, name)
    # and each job alone gives the bits it gives inside the group
    for (W, u0, G), grouped in zip(cases[:3], runs[0][0][:3]):
        alone = Job(W, u0)
        assert refresh([alone]) == 0
        assert torch.equal(alone.what, grouped.what) and torch.equal(alone.sigma, grouped.sigma)


class _Stack(nn.Module):
    def __init__(self, sizes):
        super().__init__()
        self.layers = nn.ModuleList([nn.Linear(k, m) for m, k in sizes])


def test_seventy_layers_are_each_refreshed_exactly_once():
    """More layers than one call holds (32), through the host class that splits them: after construction with n_init = 1 every
    layer's v, u, sigma and weight are ONE refresh of its own W and initial u (a layer refreshed twice, or not at all, misses
    these bounds by orders of magnitude)."""
    from txt2vid_amd.gan.spectral import SpectralNorm, initial_u
    torch.manual_seed(11)
    sizes = [(3 + i % 7, 20 + 13 * i) for i in range(70)]
    net = _Stack(sizes).to(DEV)
    Ws = [l.weight.detach().cpu().clone() for l in net.layers]
    sn = SpectralNorm([net], n_init=1, seed=5)
    assert len(sn.params) == 70 and len(sn._refresh_calls) == 3
    gen = torch.Generator().manual_seed(5)
    torch.cuda.synchronize()
    for i, W in enumerate(Ws):
        u0 = initial_u(W.shape[0], gen)
        job = Job(W, u0)
        job.v, job.u, job.sigma, job.what, job.w = sn.v[i], sn.u[i], sn.sigma[i], sn.params[i].detach(), sn.orig[i]
        check_refresh(job, W, u0)
    assert set(sn.sigmas()) == set(sn.names) and all(s > 0 for s in sn.sigmas().values())
    # the projection over the same 70 layers (three calls): every gradient mapped once, every weight restored to its master
    gg = torch.Generator().manual_seed(6)
    Gs = [torch.randn(W.shape, generator=gg) for W in Ws]
    before = [(p.detach().cpu().clone(), u.cpu().clone(), v.cpu().clone(), float(s.item()))
              for p, u, v, s in zip(sn.params, sn.u, sn.v, sn.sigma)]
    for p, G in zip(sn.params, Gs):
        p.grad = G.to(DEV)
    sn.project_grads()
    torch.cuda.synchronize()
    assert len(sn._project_calls) == 3
    for i, (W, G) in enumerate(zip(Ws, Gs)):
        ref, b = S.phase_project(G, *before[i])
        _within('dW %d' % i, sn.params[i].grad, ref, b)
        assert torch.equal(sn.params[i].detach().cpu(), W)


def test_zero_matrix_gives_finite_state():
    """t = 0: v = 0 / eps = 0, s = 0, u = 0, sigma = 0 — which divides by 1 (What = W = 0, G unchanged), as the header documents."""
    W, u0, G = S.make_case(8, 81, seed=3)
    job = Job(torch.zeros_like(W), u0, G)
    assert refresh([job]) == 0
    for t in (job.u, job.v, job.sigma, job.what):
        assert bool(torch.isfinite(t).all()) and not bool(t.any())
    assert project([job]) == 0
    assert torch.equal(job.g.cpu(), G)


def test_convergence_to_the_largest_singular_value():
    """W = 3 a b^T + noise (sigma_2 <= sigma_1 / 2; test_sn_cpu checks the float64 iteration against svdvals). After 30 kernel
    refreshes sigma is compared with the float64 iteration from the same fp32 (W, u0), which has converged to sigma_1 (its error
    shrinks by (sigma_2 / sigma_1)^2 <= 1/4 per refresh). Bound (derived): the 30th refresh alone, from the kernel's own u of the
    29th, is within e_sigma of the exact refresh of that u (`phase_v` / `phase_u_sigma`). That exact refresh differs from sigma_1
    by at most sigma_1 d^2, d the direction error of the vectors: sigma = u . W v is stationary at the singular pair, and d is
    at most the per-refresh errors |b_u|_2 + |b_v|_2 summed with the contraction 1/4: d <= (|b_u|_2 + |b_v|_2) / (1 - 1/4)."""
    for (M, K), seed in zip([(67, 129), (96, 2600)], (1, 2)):
        W, u0 = S.low_rank_case(M, K, seed)
        sv = torch.linalg.svdvals(W.double())
        assert float(sv[1]) <= 0.5 * float(sv[0])
        job = Job(W, u0)
        for _ in range(29):
            assert refresh([job]) == 0
        u29 = job.u.cpu().clone()
        assert refresh([job]) == 0
        _, _, ref, _ = S.refresh_ref(W, u0, n_iter=30)
        _, bv = S.phase_v(W, u29)
        _, bu, _, e_sigma = S.phase_u_sigma(W, job.v.cpu())
        d = (float(bu.norm()) + float(bv.norm())) / 0.75
        bound = e_sigma + ref * d * d
        err = abs(float(job.sigma.item()) - ref)
        print('[%d, %d]: sigma %.9g, float64 %.9g, |delta| / bound = %.4f' % (M, K, float(job.sigma.item()), ref, err / bound))
        assert err <= bound


# ------------------------------------------------------------------------------------------------ helpers for the runs
def pour(module):
    module.load_state_dict({k: O.recipe_tensor(k, v.shape) for k, v in module.state_dict().items()})
    return module.to(DEV)


def make(sn=False, discrim_steps=1, n_power_iterations=1):
    """B=4 unconditional 64x64 set-up of the step tests (recipe weights, RSGAN + GP 0.5, Adam), as tests/test_ema_gpu.py."""
    from txt2vid_amd.models.tganv2.gen import MultiScaleGen
    from txt2vid_amd.models.tganv2.discrim import MultiScaleDiscrim
    from txt2vid_amd.gan.cond_gan import CondGan
    from txt2vid_amd.gan.losses import MixedGanLoss, RSGANLoss
    from txt2vid_amd.gan.spectral import SpectralNorm, attach
    from txt2vid_amd.optim import Adam
    gen = pour(MultiScaleGen(width=64, height=64, num_channels=1)).train()
    dis = pour(MultiScaleDiscrim(num_channels=1)).train()
    gan = CondGan(gen=gen, discrims=[dis], discrim_names=['video'])
    losses = MixedGanLoss(g_loss=RSGANLoss(), d_loss=RSGANLoss())
    optD = Adam([{'params': dis.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    optG = Adam([{'params': gen.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    if sn:
        attach(gan, optD, SpectralNorm([dis], n_power_iterations=n_power_iterations, seed=9))

    class Prm(object):
        frame_sizes = [8, 16, 32, 64]
        subsample_input = True
        gen_steps = 1
        gp_lambda = 0.5
        no_mean_discrim_loss = no_mean_gen_loss = True
    Prm.discrim_steps = discrim_steps
    return gan, optD, optG, losses, Prm()


def seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


def batch():
    return (torch.rand(4, 16, 1, 64, 64) * 2 - 1).permute(0, 2, 1, 3, 4).contiguous().to(DEV)


def close(a, b, rtol, atol):
    """The comparison of tests/test_models_gpu.py (atol relative to the tensor's scale)."""
    a, b = a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy()
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol * max(1.0, float(np.abs(b).max())))


def _d_pass(gan, prm, x, losses):
    """One discriminator forward + backward (grouped pyramid path, gradient penalty) without an update: (loss, {name: grad})."""
    from txt2vid_amd import functional as TF
    from txt2vid_amd.gan.trainer import multiscale_data
    dis = gan.discrims[0]
    TF.set_grad_sink(None)                                   # plain autograd gradients, whatever an earlier test armed
    for p in dis.parameters():
        p.grad = None
    seed(77)
    xs, _ = multiscale_data(x, None, prm.frame_sizes, prm.subsample_input)
    with torch.no_grad():
        fake = gan(TF.draws.z(x.size(0), gan.gen.latent_size, DEV))
    loss = gan.discrim_step(real=xs, fake=[f.detach() for f in fake], cond=None, loss=losses.discrim_loss, gp_lambda=prm.gp_lambda)
    loss.backward()
    TF.grad_sink_flush()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in dis.named_parameters()}


# ------------------------------------------------------------------------------------------------ 2. model level
def test_the_discriminator_multiplies_with_the_normalised_weights_everywhere():
    """After construction (15 refreshes) and after a further `refresh()`, a plain discriminator whose weights are a copy of What
    gives bit-identical loss and weight gradients (before projection) on the grouped pyramid path with the gradient penalty: no
    kernel reads a stale or mis-keyed packed copy."""
    from txt2vid_amd import functional as TF
    gan, optD, optG, losses, prm = make(sn=True)
    sn, dis = gan.discrim_sn, gan.discrims[0]
    seed(1)
    x = batch()
    _d_pass(gan, prm, x, losses)                             # fills the packed-weight caches with the current What
    # a discriminator update by hand: W moves, refresh() re-normalises, the optimiser's re-pack follows
    with torch.no_grad():
        for p, w in zip(sn.params, sn.orig):
            TF.copy_into((w * 1.25 + 0.01).contiguous(), p.detach())
    sn.refresh()
    TF.bump_weight_epoch(sn.params)
    TF.repack_params(sn.params)
    torch.cuda.synchronize()
    for p, w, s in zip(sn.params, sn.orig, sn.sigma):
        ref, b = S.phase_scale(w.cpu(), float(s.item()))
        assert bool(((p.detach().cpu().double() - ref).abs() <= b).all())
    loss_sn, grads_sn = _d_pass(gan, prm, x, losses)
    plain, _, _, _, _ = make(sn=False)
    plain.gen.load_state_dict(gan.gen.state_dict())
    plain.discrims[0].load_state_dict({k: v.detach().clone() for k, v in dis.state_dict().items()})
    TF.bump_weight_epoch()
    loss_plain, grads_plain = _d_pass(plain, prm, x, losses)
    assert torch.equal(loss_sn, loss_plain), (float(loss_sn), float(loss_plain))
    for k in grads_plain:
        assert torch.equal(grads_sn[k], grads_plain[k]), k


def _fresh_pack_matches(params):
    """Every persistent packed copy of `params` (plain and fused fp32 variants) equals a fresh pack of the parameter's current
    contents. Returns how many copies were compared."""
    import ctypes as C
    from txt2vid_amd import functional as TF
    n = 0
    for p in params:
        for key, rec in TF._pack_cache.get(id(p), {}).items():
            if rec.ref() is not p or rec.kind == 'bf16':
                continue
            w, Cout, Cin, T, taps, mode, rows, cols, ro, co = rec.job
            taps_c = (C.c_int32 * len(taps))(*taps)
            if rec.kind == 'fused':
                wp = rec.buf
                fresh = torch.zeros_like(wp)
                TF.check(TF.lib().t2v_pack_weight_into(TF._p(w), TF._p(fresh), Cout, Cin, T, taps_c, len(taps), mode, rows, cols, ro, co,
                                                       TF._stream()), 't2v_pack_weight_into')
                mask = fresh != 0
                assert bool(mask.any()) and torch.equal(fresh[mask], wp[mask]), key
            else:
                shape5, _, mode = key
                fresh = torch.empty_like(rec.buf)
                TF.check(TF.lib().t2v_pack_weight(TF._p(p.detach().view(shape5)), TF._p(fresh), shape5[0], shape5[1], T, taps_c,
                                                  len(taps), mode, TF._stream()), 't2v_pack_weight')
                assert torch.equal(fresh, rec.buf), key
            n += 1
    return n


def _run(graphed, iters=3):
    from txt2vid_amd.gan.trainer import GraphedTrainStep, TrainStep
    parts = make(sn=True, discrim_steps=2)
    gan, optD, optG, losses, prm = parts
    sn = gan.discrim_sn
    seed(100)
    gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (4, 1, 16, 64, 64), warmup=2) if graphed else None
    out = []
    for i in range(iters):
        x = batch()
        if graphed:
            lD, lG = gs.step(x)
        else:
            lD, lG, _, _ = TrainStep(gan, optD, optG, losses, prm, DEV).run(x)
        torch.cuda.synchronize()
        # invariants of every iteration, eager or replayed: `weight` = W / sigma, and every packed copy is a pack of it
        for p, w, s in zip(sn.params, sn.orig, sn.sigma):
            ref, b = S.phase_scale(w.cpu(), float(s.item()))
            assert bool(((p.detach().cpu().double() - ref).abs() <= b).all())
        assert _fresh_pack_matches(sn.params) >= len(sn.params)
        out.append((float(lD), float(lG), [w.clone() for w in sn.orig], [u.clone() for u in sn.u], [v.clone() for v in sn.v],
                    [float(s.item()) for s in sn.sigma]))
    if graphed:
        assert gs.graphs is not None
    return sn, out


def test_graph_replay_matches_eager_with_two_discriminator_steps():
    """Three iterations of `GraphedTrainStep` (two eager, one captured and replayed) against three eager ones, --discrim_steps 2:
    two refreshes per iteration in every Python pass, and inside each run, after every iteration, `weight` = W / sigma and every
    packed copy is a fresh pack of it (`_run`). Across the runs the losses agree as test_models_gpu's replay test asks of two runs
    of the same code (5e-6 on the eager iterations, 5e-4 on the replayed one). The master W of the two runs may differ by what
    Adam can do with gradients that differ in their last bits: a bias-corrected update moves a weight by at most
    lr (1 - b1) / (1 - b1^t) sqrt((1 - b2^t) / (1 - b2)) <= 1.25 lr for t <= 6, b = (0.5, 0.999), so after k updates two runs are
    within 2 * 1.25 * lr * k of each other — far below |W - W / sigma|, which a run that lost its master copy would show. u and
    v are unit vectors; sigma is printed for both runs."""
    _run(False, iters=1)                                     # burn-in (see test_models_gpu.test_graph_replay_matches_eager)
    sn_e, eager = _run(False)
    assert sn_e.refreshes == 2 * 3
    sn_g, graphed = _run(True)
    assert sn_g.refreshes == 2 * 3                           # two eager passes and the capture pass; the replay runs the captured ones
    lr = 2e-4
    for i, (a, b) in enumerate(zip(eager, graphed)):
        print('iteration %d: eager %r | graphed %r' % (i, a[:2], b[:2]))
        tol = 5e-6 if i < 2 else 5e-4
        assert abs(a[0] - b[0]) < tol and abs(a[1] - b[1]) < tol, (i, a[:2], b[:2])
        worst = 0.0
        for k, wa, wb in zip(sn_e.names, a[2], b[2]):
            worst = max(worst, float((wa - wb).abs().max()))
        print('    max |W eager - W graphed| = %.3g (bound %.3g); sigma[0] %.6g | %.6g' % (worst, 2 * 1.25 * lr * 2 * (i + 1),
                                                                                          a[5][0], b[5][0]))
        assert worst <= 2 * 1.25 * lr * 2 * (i + 1)
    for run in (eager, graphed):
        for k in range(len(sn_e.names)):
            assert not torch.equal(run[2][2][k], run[0][2][k])                  # W moved between iterations 1 and 3
            assert abs(float(run[2][3][k].double().norm()) - 1.0) < 1e-5 and abs(float(run[2][4][k].double().norm()) - 1.0) < 1e-5


def _counted(run):
    from txt2vid_amd import functional as TF
    l = TF.lib()
    names = ('t2v_sn_refresh', 't2v_sn_project', 't2v_sn_ws_floats')
    orig = {n: getattr(l, n) for n in names}
    calls = {n: 0 for n in names}

    def wrap(n):
        def f(*a):
            calls[n] += 1
            return orig[n](*a)
        return f
    try:
        for n in names:
            setattr(l, n, wrap(n))
        out = run()
    finally:
        for n in names:
            setattr(l, n, orig[n])
    return calls, out


def _three_iterations(gan, optD, optG, losses, prm):
    from txt2vid_amd.gan.trainer import GraphedTrainStep
    seed(100)
    gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (4, 1, 16, 64, 64), warmup=2)
    for _ in range(3):
        gs.step(batch())
    torch.cuda.synchronize()
    assert gs.graphs is not None
    return gan, optD


def test_off_means_off():
    """Without --D_sn three iterations (two eager, one captured and replayed) call none of the new entry points and the optimiser
    carries no hook; with it every discriminator update makes one projection and one refresh call (20 layers: one call each)."""
    calls, (gan, optD) = _counted(lambda: _three_iterations(*make(sn=False)))
    assert calls == {'t2v_sn_refresh': 0, 't2v_sn_project': 0, 't2v_sn_ws_floats': 0}
    assert optD.weight_hook is None and gan.discrim_sn is None
    parts = make(sn=True)
    calls, (gan, optD) = _counted(lambda: _three_iterations(*parts))
    assert optD.weight_hook is gan.discrim_sn
    assert calls['t2v_sn_refresh'] == 3 and calls['t2v_sn_project'] == 3
    assert gan.discrim_sn.launches_per_update == 3 + 5 + 1


def test_one_discriminator_step_against_the_oracle():
    """One D step with gp_lambda = 0.5 against `oracle.tganv2_oracle.discrim_loss` evaluated on a parameter dict whose weights
    are W / sigma, built with torch autograd from the master W and the kernel's u, v (`sn_cases.normalised_param_dict`): the loss
    within 2e-4 and every dL/dW norm within rtol 3e-3 — the bounds tests/test_models_gpu.py asserts for the un-normalised step
    (test_teacher_forced_steps_vs_oracle, test_first_step_grad_norms_vs_reference_golden). The product's gradients are what the
    optimiser would consume: backward, the sink's flush, then `project_grads()`."""
    from txt2vid_amd import functional as TF
    from txt2vid_amd.gan.trainer import multiscale_data
    gan, optD, optG, losses, prm = make(sn=True)
    sn, dis = gan.discrim_sn, gan.discrims[0]
    TF.set_grad_sink(None)
    seed(7)
    x = batch()
    xs, _ = multiscale_data(x, None, prm.frame_sizes, True)
    with torch.no_grad():
        fake = [f.detach() for f in gan(torch.randn(4, gan.gen.latent_size).to(DEV))]
    for p in dis.parameters():
        p.grad = None
    st_t, st_n, st_r = torch.get_rng_state(), np.random.get_state(), random.getstate()
    lD = gan.discrim_step(real=xs, fake=fake, cond=None, loss=losses.discrim_loss, gp_lambda=0.5)
    lD.backward()
    TF.grad_sink_flush()
    sn.project_grads()
    torch.cuda.synchronize()
    got = {k: float(p.grad.double().norm()) for k, p in zip(sn.names, sn.params)}
    for p, w in zip(sn.params, sn.orig):
        assert torch.equal(p.detach(), w)                     # the update that follows runs on the master W
    # the oracle, on the CPU, same draws (the GP alphas)
    torch.set_rng_state(st_t)
    np.random.set_state(st_n)
    random.setstate(st_r)
    P = {k: v.detach().cpu().clone() for k, v in dis.state_dict().items()}
    state = {}
    for k, w, u, v in zip(sn.names, sn.orig, sn.u, sn.v):
        state[k[2:]] = (w.detach().cpu().clone().requires_grad_(True), u.cpu().clone(), v.cpu().clone())
    P = S.normalised_param_dict(P, state, list(state))
    lo = O.discrim_loss(P, 'single_discrim.', [t.cpu() for t in xs], [t.cpu() for t in fake], gp_lambda=0.5)
    lo.backward()
    print('lossD %.7f vs oracle %.7f' % (float(lD), float(lo)))
    assert abs(float(lD) - float(lo)) < 2e-4
    worst = 0.0
    for k in sn.names:
        want = float(state[k[2:]][0].grad.double().norm())
        rel = abs(got[k] - want) / max(want, 1e-30)
        worst = max(worst, rel)
        print('    %-60s |dL/dW| %.6e vs %.6e (rel %.2e)' % (k, got[k], want, rel))
    for k in sn.names:
        want = float(state[k[2:]][0].grad.double().norm())
        assert abs(got[k] - want) <= 3e-3 * want, (k, got[k], want)
    print('worst relative difference of a gradient norm: %.3e' % worst)


def test_master_weights_and_vectors_evolve_as_the_reference_predicts():
    """Two eager iterations with --discrim_steps 2 and plain SGD on the discriminator (lr 1e-2, no momentum: W' = W - lr dL/dW is
    linear in the gradient, so the prediction carries a bound). Around every discriminator update the hook's inputs are recorded:
    G = dL/dWhat as the optimiser finds it after the flush, What, W, u, v, sigma. Predicted in float64 (tests/sn_cases.py):
        dW = project_ref(G, What, u, v, sigma) ; W' = W - lr dW ; (v', u', sigma') = one refresh of (W', u)
    Bounds (derived): the projection within `phase_project`'s b; the update adds the rounding of lr to fp32, of lr dW and of the
    subtraction, |W' error| <= lr b + 3 E (|W| + lr (|dW| + b)); v', u', sigma', What' from the kernel's own W' at the op-level bounds
    (`check_refresh`). A wrong sign or scale of the projection, a gradient projected twice, a refresh that reads the wrong buffer or
    an update applied to What instead of W each miss these bounds by orders of magnitude. Four updates are checked."""
    from txt2vid_amd.gan.trainer import TrainStep
    from txt2vid_amd.gan.spectral import attach, SpectralNorm
    from txt2vid_amd.optim import SGD
    gan, _, optG, losses, prm = make(sn=False, discrim_steps=2)
    dis = gan.discrims[0]
    lr = 1e-2
    optD = SGD([{'params': dis.parameters()}], lr=lr, momentum=0.0)
    sn = SpectralNorm([dis], seed=9)
    attach(gan, optD, sn)
    rec = []
    project, refresh_ = sn.project_grads, sn.refresh

    def recording_project():
        torch.cuda.synchronize()
        rec.append([[t.detach().cpu().clone() for t in ts] for ts in
                    ([p.grad for p in sn.params], sn.params, sn.orig, sn.u, sn.v, sn.sigma)])
        project()

    def recording_refresh(touched=()):
        out = refresh_(touched)
        torch.cuda.synchronize()
        rec[-1].append([[t.detach().cpu().clone() for t in ts] for ts in (sn.orig, sn.u, sn.v, sn.sigma, sn.params)])
        return out
    sn.project_grads, sn.refresh = recording_project, recording_refresh
    seed(100)
    for _ in range(2):
        TrainStep(gan, optD, optG, losses, prm, DEV).run(batch())
    torch.cuda.synchronize()
    assert len(rec) == 4 and sn.refreshes == 4
    worst = 0.0
    for n, (G, What, W, u, v, sg, after) in enumerate(rec):
        W2, u2, v2, sg2, What2 = after
        for i, k in enumerate(sn.names):
            M = W[i].shape[0]
            dW, b = S.phase_project(G[i].reshape(M, -1), What[i].reshape(M, -1), u[i], v[i], float(sg[i]))
            Wd = W[i].double().reshape(M, -1)
            pred = Wd - lr * dW
            bound = lr * b + 3 * S.E * (Wd.abs() + lr * (dW.abs() + b))
            err = (W2[i].double().reshape(M, -1) - pred).abs()
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            assert bool((err <= bound).all()), (n, k, float(err.max()), float(bound.max()))
            # the refresh, from the kernel's own W' and the u it started from
            job = Job.__new__(Job)
            job.M, job.K = M, Wd.shape[1]
            job.w, job.u, job.v, job.sigma, job.what = W2[i].reshape(M, -1), u2[i], v2[i], sg2[i], What2[i].reshape(M, -1)
            if i in (0, 5, len(sn.names) - 1) or n == 3:
                check_refresh(job, W2[i].reshape(M, -1), u[i])
    print('master weights: worst |delta| / bound = %.4f' % worst)


def test_replicas_stay_identical_with_two_ranks():
    """Data parallel (tools/dp_check.py --D_sn, the pattern of tests/test_dp_gpu.py): after five graph-replayed iterations the
    weights, the master weights, u, v and sigma are identical on both ranks, and differ from a solo run. Over RCCL with one rank
    per GPU where two devices are visible; otherwise rehearsed over gloo with both ranks on device 0."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0')
    if torch.cuda.device_count() < 2:
        env.update(T2V_DIST_BACKEND='gloo', T2V_SINGLE_DEVICE='1')
    else:
        env.pop('T2V_DIST_BACKEND', None)
        env.pop('T2V_SINGLE_DEVICE', None)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', '29537', os.path.join(ROOT, 'tools', 'dp_check.py'), '--D_sn']
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = p.stdout.decode(errors='replace')
    assert p.returncode == 0, out[-3000:]
    line = [l for l in out.splitlines() if l.startswith('DP_CHECK')]
    assert line and 'identical after 5 iterations: True' in line[0] and 'spectral norm' in line[0], out[-2000:]


# ------------------------------------------------------------------------------------------------ 3. command line
def test_cli_round_trip(tmp_path):
    """tools/cfg/synth.json's data set (64x64x1 here, one batch per epoch so that a resumed run meets the batch the first run met
    next: the epoch's permutation and every draw of the iteration come from the generator states the checkpoint carries), eager
    launches, the logged losses those of the last iteration alone (--loss_window_size 1):
      * a checkpoint written WITHOUT the flag loads into a --D_sn run: its weights are taken as W, 15 power iterations run;
      * that run writes a checkpoint with the state after iteration 3 (`weight` = W / sigma, unit u) and goes on to iteration 4;
      * resuming the checkpoint reproduces iteration 4's logged losses exactly; the state the resumed run starts from (W, u, v,
        sigma of every layer, and `weight`) is the saved one bit for bit;
      * the checkpoint is refused without --D_sn, with a message that names the flag."""
    import re
    with open(os.path.join(ROOT, 'tools', 'cfg', 'synth.json')) as f:
        spec = json.load(f)
    spec.setdefault('args', {}).update({'num_frames': 16, 'length': 8})
    cfg = str(tmp_path / 'synth.json')
    with open(cfg, 'w') as f:
        json.dump(spec, f)
    base = ['--data', cfg, '--num_channels', '1', '--cuda', '--frame_sizes', '8', '16', '32', '64', '--D_names', 'video',
            '--G_lr', '0.0002', '--D_lr', '0.0002', '--D_beta1', '0.5', '--D_beta2', '.999', '--G_beta1', '0.5', '--G_beta2', '.999',
            '--D_loss', 'txt2vid.gan.losses.RSGANLoss', '--init_method', 'xavier', '--discrim_steps', '1', '--seed', '100',
            '--gp_lambda', '.5', '--subsample_input', '--workers', '0', '--log_period', '1', '--loss_window_size', '1', '--no_graph',
            '--G', 'txt2vid.models.tganv2.gen.MultiScaleGen', '--D', 'txt2vid.models.tganv2.discrim.MultiScaleDiscrim',
            '--dont_use_sent', '--batch_size', '8', '--save_example_period', '0']

    def run(args, ok=True):
        p = subprocess.run([sys.executable, '-m', 'txt2vid_amd.train.gan'] + base + args, cwd=ROOT, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=600)
        out = p.stdout.decode(errors='replace')
        assert (p.returncode == 0) == ok, out[-3000:]
        return out

    def losses_of(log, it):
        m = re.search(r'Iter %d, Loss_D: (\S+) Loss_G: (\S+)' % it, log)
        assert m, log[-2000:]
        return m.group(1), m.group(2)

    def one(pattern):
        found = glob.glob(pattern)
        assert len(found) == 1, (pattern, found)
        return found[0]
    out0 = str(tmp_path / 'out0')
    run(['--out', out0, '--out_samples', str(tmp_path / 's0'), '--epochs', '1', '--save_model_period', '1'])
    plain = one(os.path.join(out0, 'iter_1_lossG_*'))
    assert 'discrim_sn' not in torch.load(plain, map_location='cpu', weights_only=False)
    out1 = str(tmp_path / 'out1')
    log1 = run(['--out', out1, '--out_samples', str(tmp_path / 's1'), '--D_sn', '--weights', plain, '--epochs', '4',
                '--save_model_period', '1'])
    assert '15 initial power iterations' in log1
    ck3, ck4 = one(os.path.join(out1, 'iter_3_lossG_*')), one(os.path.join(out1, 'iter_4_lossG_*'))
    sd = torch.load(ck3, map_location='cpu', weights_only=False)
    state = sd['discrim_sn']
    assert len(state) == 4 * 20
    for k in [k[:-len('_orig')] for k in state if k.endswith('_orig')]:
        W, u, v, s = (state[k + sfx] for sfx in ('_orig', '_u', '_v', '_sigma'))
        assert k.startswith('0.single_discrim.') and u.shape == (W.shape[0],) and v.shape == (W[0].numel(),) and s.shape == (1,)
        assert float(s) > 0 and abs(float(u.double().norm()) - 1) < 1e-5
        ref, b = S.phase_scale(W, float(s))
        assert bool(((sd['video'][k[2:]].double() - ref).abs() <= b).all()), k          # the saved `weight` is W / sigma
    log = run(['--out', str(tmp_path / 'o3'), '--out_samples', str(tmp_path / 's3'), '--weights', ck3, '--epochs', '1'], ok=False)
    assert '--D_sn' in log and 'ValueError' in log
    out2 = str(tmp_path / 'out2')
    log2 = run(['--out', out2, '--out_samples', str(tmp_path / 's2'), '--D_sn', '--weights', ck3, '--epochs', '1',
                '--save_model_period', '1'])
    assert 'state from the checkpoint' in log2
    first, resumed = losses_of(log1, 4), losses_of(log2, 1)
    print('iteration 4 of the first run: Loss_D %s Loss_G %s | resumed: Loss_D %s Loss_G %s' % (first + resumed))
    assert first == resumed
    # the state a resumed run starts from is the saved one bit for bit, `weight` untouched and no refresh run
    from txt2vid_amd.gan.spectral import SpectralNorm
    from txt2vid_amd.models.tganv2.discrim import MultiScaleDiscrim
    dis = MultiScaleDiscrim(num_channels=1)
    dis.load_state_dict(sd['video'])
    dis.to(DEV)
    sn = SpectralNorm([dis], state=state)
    torch.cuda.synchronize()
    assert sn.refreshes == 0 and list(sn.state_dict()) == list(state)
    for k, t in sn.state_dict().items():
        assert torch.equal(t.cpu(), state[k]), k
    for k, t in dis.state_dict().items():
        assert torch.equal(t.cpu(), sd['video'][k]), k
    # after the resumed iteration: the master weights of the two runs are one Adam update from the same state apart. The first
    # backward pass of a process accumulates its independent gradient contributions in another order than later ones
    # (test_models_gpu.test_graph_replay_matches_eager), so the gradients differ in their last bits and the updates by at most
    # 2 * 1.25 * lr (see test_graph_replay_matches_eager_with_two_discriminator_steps); the weights did move
    want = torch.load(ck4, map_location='cpu', weights_only=False)['discrim_sn']
    got = torch.load(one(os.path.join(out2, 'iter_1_lossG_*')), map_location='cpu', weights_only=False)['discrim_sn']
    worst = max(float((want[k] - got[k]).abs().max()) for k in want if k.endswith('_orig'))
    print('max |W first run - W resumed| after iteration 4: %.3g' % worst)
    assert worst <= 2 * 1.25 * 2e-4
    assert not torch.equal(want['0.single_discrim.fc_uncond.weight_orig'], state['0.single_discrim.fc_uncond.weight_orig'])
