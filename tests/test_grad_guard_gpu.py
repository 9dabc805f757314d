"""GPU: gradient clipping and the non-finite guard inside the replayed graph (--grad_guard / --D_clip / --G_clip) —
  kernels:     the norm against float64, the coefficient and the counters, the guarded launches are the existing ones called
               with the float product, and every place a NaN can hide skips the step and leaves every bit alone;
  optimisers:  clipped Adam / SGD against torch.optim preceded by clip_grad_norm_, and the composition with --D_sn;
  iterations:  the decision is taken at replay time, clipping that does not bite changes no bit, clipping that bites does,
               off means off, a re-capture keeps addresses and counts, and the command line round trip."""
import glob
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import guard_cases as G
import test_ema_gpu as TE                  # (its set-up helpers: make, seed)
import test_lr_sched_gpu as TL             # (its job sets: _job_sets, _jobs, _clone, batches)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 2e-4
B1, B2, ADAM_EPS = 0.5, 0.999, 1e-8


def _bits(t):
    return t.detach().view(torch.int32).clone()


def _state(coef=1.0, skip=0.0, norm=0.0, steps=0.0, skipped=0.0, clipped=0.0):
    return torch.tensor([coef, skip, norm, steps, skipped, clipped, 0.0, 0.0], dtype=torch.float32).to(DEV)


def _measure(items, gscale, clip, st):
    """sumsq + decision over the job list, as gan.grad_guard.OptGuard.measure issues them. Returns the partials."""
    from txt2vid_amd import functional as TF
    n = sum((t[0].numel() + 4095) // 4096 for t in items)
    partials = torch.full((n + 3,), -7.0).to(DEV)                                  # (three slots past the end: never written)
    assert TF.lib().t2v_grad_sumsq_multi(TL._jobs(items), len(items), gscale, TF._p(partials), TF._stream()) == 0
    assert TF.lib().t2v_grad_guard(TF._p(partials), n, clip, TF._p(st), TF._stream()) == 0
    torch.cuda.synchronize()
    assert partials[n:].tolist() == [-7.0] * 3
    return partials[:n].clone()


@pytest.fixture(scope='module')
def job_sets():
    return TL._job_sets()


# ------------------------------------------------------------------------------------------------ 1. the norm
@pytest.mark.parametrize('gscale', [1.0, 0.5])
def test_norm_against_float64(job_sets, gscale):
    """norm = (float)sqrt(sum of the chunk partials in double) against sqrt(sum((gscale * g)^2)) in float64 on the CPU.
    Bound (derived, not measured): a thread adds at most 17 squares serially (16 from four float4 loads, one more where a chunk
    shorter than 4096 has a scalar tail), the wave64 shuffle adds 6 levels, the four waves 2: 25 additions of positive terms;
    every term carries the rounding of g * gscale twice and of the square once (3). 28 roundings x 2^-24 = 1.7e-6 relative on the
    sum of squares; the partials are added exactly enough in double; the square root halves it (0.84e-6) and the final rounding
    to float adds 6e-8: <= 2e-6. Two calls on the same inputs give the same bits."""
    for items in job_sets:
        st = _state()
        part = _measure(items, gscale, 0.0, st)
        got = st.tolist()
        want = G.norm64([t[1] for t in items], gscale)
        rel = abs(got[2] - want) / want
        print('%d jobs, gscale %g: norm %.9g float64 %.17g rel %.3g' % (len(items), gscale, got[2], want, rel))
        assert rel <= 2e-6
        assert got[:2] == [1.0, 0.0] and got[3:] == [1.0, 0.0, 0.0, 0.0, 0.0]
        st2 = _state()
        part2 = _measure(items, gscale, 0.0, st2)
        assert torch.equal(_bits(part), _bits(part2)) and torch.equal(_bits(st), _bits(st2))
        # every chunk's partial on its own, in float64 (the chunk order is the job order)
        ref = torch.cat([(c.double() * float(np.float32(gscale))).pow(2).sum().reshape(1)
                         for t in items for c in t[1].cpu().split(4096)])
        assert ref.numel() == part.numel()
        assert bool(((part.cpu().double() - ref).abs() <= 1.7e-6 * ref).all())


# ------------------------------------------------------------------------------------------------ 2. coefficient and counters
def test_coef_and_counters(job_sets):
    """C above, about at and well below the measured norm; then clip = 0. coef is the fp32 formula on the device's own norm
    (exact, or 1 ulp for the division), exactly 1.0 when the norm is below C; the counts advance as defined."""
    for items in job_sets:
        probe = _state()
        _measure(items, 1.0, 0.0, probe)
        norm = np.float32(probe[2].item())
        st = _state()
        seen = []
        for clip in (float(norm) * 4.0, float(np.nextafter(norm, np.float32(np.inf))), float(norm), float(norm) * 0.01, 0.0):
            _measure(items, 1.0, clip, st)
            row = st.tolist()
            want = G.coef32(row[2], clip) if clip > 0 else np.float32(1.0)
            print('%d jobs: C %.9g norm %.9g -> coef %.9g (formula %.9g), counts %s' % (len(items), clip, row[2], row[0], want, row[3:6]))
            assert np.float32(row[2]) == norm and row[1] == 0.0
            assert G.within_one_ulp(row[0], want)
            assert (row[0] == 1.0) == bool(want == np.float32(1.0))
            if clip == 0.0 or norm + np.float32(1e-6) <= np.float32(clip):
                assert row[0] == 1.0
            seen.append(row)
        assert [r[3] for r in seen] == [1.0, 2.0, 3.0, 4.0, 5.0]                    # steps
        assert [r[4] for r in seen] == [0.0] * 5                                   # skipped
        assert seen[0][0] == 1.0 and seen[3][0] < 0.0101 and seen[4][0] == 1.0
        clipped = 0.0
        for r in seen:
            clipped += 1.0 if r[0] < 1.0 else 0.0
            assert r[5] == clipped and r[6:] == [0.0, 0.0]
        assert seen[4][5] >= 1.0                                                   # (C = norm / 100 did clip)


# ------------------------------------------------------------------------------------------------ 3. guarded = existing with the product
@pytest.mark.parametrize('with_sched', [False, True])
@pytest.mark.parametrize('with_step_dev', [False, True])
@pytest.mark.parametrize('c', [1.0, 0.37])
def test_guarded_adam_is_adam_with_the_product(job_sets, c, with_step_dev, with_sched):
    """t2v_adam_multi_guard(gscale, state {coef = c}) against t2v_adam_multi(_sched) with gscale' = float32(gscale) * float32(c):
    p, m and v bit for bit; the launch only reads the state."""
    from txt2vid_amd import functional as TF
    l = TF.lib()
    step = 3
    bc1, bc2 = 1.0 - B1 ** step, 1.0 - B2 ** step
    step_dev = torch.tensor([float(step), bc1, bc2], dtype=torch.float32).to(DEV) if with_step_dev else None
    host_bc = (7.0, 7.0) if with_step_dev else (bc1, bc2)
    gscale = 0.5
    product = float(np.float32(gscale) * np.float32(c))
    st = _state(c, 0.0, 12.5, 4.0, 1.0, 2.0)
    sched = torch.tensor([9.0, 0.37], dtype=torch.float32).to(DEV) if with_sched else None
    for items in job_sets:
        a, b = TL._clone(items), TL._clone(items)
        assert l.t2v_adam_multi_guard(TL._jobs(a), len(a), LR, TF._p(sched), B1, B2, ADAM_EPS, host_bc[0], host_bc[1], gscale,
                                      TF._p(step_dev), TF._p(st), TF._stream()) == 0
        if with_sched:
            assert l.t2v_adam_multi_sched(TL._jobs(b), len(b), LR, TF._p(sched), B1, B2, ADAM_EPS, host_bc[0], host_bc[1], product,
                                          TF._p(step_dev), TF._stream()) == 0
        else:
            assert l.t2v_adam_multi(TL._jobs(b), len(b), LR, B1, B2, ADAM_EPS, host_bc[0], host_bc[1], product, TF._p(step_dev),
                                    TF._stream()) == 0
        torch.cuda.synchronize()
        assert st.tolist() == [float(np.float32(c)), 0.0, 12.5, 4.0, 1.0, 2.0, 0.0, 0.0]
        for (pa, ga, ma, va), (pb, gb, mb, vb), (p0, g0, m0, v0) in zip(a, b, items):
            n = p0.numel()
            assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb), (c, n)
            assert torch.equal(ga, g0)
            assert not torch.equal(pa, p0) and not torch.equal(ma, m0) and not torch.equal(va, v0), n


@pytest.mark.parametrize('with_sched', [False, True])
@pytest.mark.parametrize('mu', [0.0, 0.5])
def test_guarded_sgd_is_sgd_with_the_product(job_sets, mu, with_sched):
    from txt2vid_amd import functional as TF
    l = TF.lib()
    sched = torch.tensor([2.0, 0.37], dtype=torch.float32).to(DEV) if with_sched else None
    for c in (1.0, 0.37):
        product = float(np.float32(0.5) * np.float32(c))
        st = _state(c, 0.0, 3.0, 1.0, 0.0, 1.0)
        for items in job_sets:
            a, b = TL._clone(items), TL._clone(items)
            assert l.t2v_sgd_multi_guard(TL._jobs(a, False), len(a), LR * 100, TF._p(sched), mu, 0.5, 0, TF._p(st), TF._stream()) == 0
            if with_sched:
                assert l.t2v_sgd_multi_sched(TL._jobs(b, False), len(b), LR * 100, TF._p(sched), mu, product, 0, TF._stream()) == 0
            else:
                assert l.t2v_sgd_multi(TL._jobs(b, False), len(b), LR * 100, mu, product, 0, TF._stream()) == 0
            torch.cuda.synchronize()
            assert st.tolist() == [float(np.float32(c)), 0.0, 3.0, 1.0, 0.0, 1.0, 0.0, 0.0]
            for (pa, ga, ma, va), (pb, gb, mb, vb), (p0, g0, m0, v0) in zip(a, b, items):
                n = p0.numel()
                assert torch.equal(pa, pb) and torch.equal(ma, mb), (c, mu, n)
                assert torch.equal(va, v0) and torch.equal(ga, g0)
                assert torch.equal(ma, m0) == (mu == 0.0) and not torch.equal(pa, p0), n


# ------------------------------------------------------------------------------------------------ 4. where a NaN can hide
# (set, job, element): element 0 of the first job; the last element of a vectorised run (the 4097-element job: its first chunk is
# 1024 float4 loads); the last element of the scalar tail of the job one float off alignment; the last element of job 69, which the
# second launch of the 70-job call covers
HIDING = [(0, 0, 0), (0, 4, 4095), (0, 6, 5000), (1, 69, -1)]


def _guarded_round(items, st, step_dev, mu_items):
    """One guarded optimiser step's launches on `items` (Adam with the device triple) and on `mu_items` (SGD, mu = 0.5)."""
    from txt2vid_amd import functional as TF
    l = TF.lib()
    _measure(items, 1.0, 0.0, st)
    assert l.t2v_adam_tick_guard(TF._p(step_dev), B1, B2, TF._p(st), TF._stream()) == 0
    assert l.t2v_adam_multi_guard(TL._jobs(items), len(items), LR, None, B1, B2, ADAM_EPS, 7.0, 7.0, 1.0, TF._p(step_dev), TF._p(st),
                                  TF._stream()) == 0
    assert l.t2v_sgd_multi_guard(TL._jobs(mu_items, False), len(mu_items), 0.01, None, 0.5, 1.0, 0, TF._p(st), TF._stream()) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize('bad', [float('nan'), float('inf'), float('-inf')])
@pytest.mark.parametrize('where', HIDING)
def test_a_single_bad_value_skips_the_step(job_sets, where, bad):
    """One NaN / inf at each hiding place: skip == 1, and after the guarded tick, Adam and SGD every p, m, v and the
    {step, bc1, bc2} triple is bitwise what it was. The next call with finite gradients is bit-identical to a twin that never
    saw the bad step."""
    which, j, e = where
    base = job_sets[which]
    adam, sgd, twin_adam, twin_sgd = (TL._clone(base) for _ in range(4))
    triple = [2.0, 1.0 - B1 ** 2, 1.0 - B2 ** 2]
    step_dev, twin_dev = (torch.tensor(triple, dtype=torch.float32).to(DEV) for _ in range(2))
    st, twin_st = _state(), _state()
    good = adam[j][1][e].item()
    adam[j][1][e] = bad                                        # the gradient of job j, element e
    before = [[_bits(t) for t in ts] for ts in adam + sgd]
    dev_before = _bits(step_dev)
    sgd_bad = [(p, adam[i][1], m, v) for i, (p, g, m, v) in enumerate(sgd)]      # (SGD reads the same gradients)
    _guarded_round(adam, st, step_dev, sgd_bad)
    row = st.tolist()
    print('%r at set %d job %d element %d: state %s' % (bad, which, j, e, row))
    assert row[0] == 1.0 and row[1] == 1.0 and not np.isfinite(row[2]) and row[3:6] == [1.0, 1.0, 0.0]
    assert torch.equal(_bits(step_dev), dev_before)
    for ts, bs in zip(adam + sgd, before):
        for k, (t, b) in enumerate(zip(ts, bs)):
            if k != 1:                                         # (the gradient itself holds the bad value)
                assert torch.equal(_bits(t), b)
    # the finite step behind it, against the twin
    adam[j][1][e] = good
    _guarded_round(adam, st, step_dev, sgd_bad)
    _guarded_round(twin_adam, twin_st, twin_dev, [(p, twin_adam[i][1], m, v) for i, (p, g, m, v) in enumerate(twin_sgd)])
    assert st.tolist()[:3] == twin_st.tolist()[:3] and st.tolist()[3:6] == [2.0, 1.0, 0.0] and twin_st.tolist()[3:6] == [1.0, 0.0, 0.0]
    assert torch.equal(_bits(step_dev), _bits(twin_dev)) and step_dev[0].item() == 3.0
    for ts, tw, bs in zip(adam + sgd, twin_adam + twin_sgd, before):
        for k, (t, w, b) in enumerate(zip(ts, tw, bs)):
            assert torch.equal(_bits(t), _bits(w))
            if k == 0:
                assert not torch.equal(_bits(t), b)            # and it moved


# ------------------------------------------------------------------------------------------------ optimiser level
SHAPES = [(5,), (4099,), (3, 7, 11), (1,)]


def _rnd(seed, *shape):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _attach(optD, optG, clip_D=None, clip_G=None):
    from txt2vid_amd.gan.grad_guard import GradGuard
    return GradGuard(clip_D, clip_G, DEV).attach(optD, optG)


def _clipped_against_torch(make_ref, make_got, clip, rtol, atol, state_key):
    from txt2vid_amd.optim import Adam
    ps0 = [_rnd(100 + i, *sh) for i, sh in enumerate(SHAPES)]
    ref = [torch.nn.Parameter(p.clone()) for p in ps0]
    got = [torch.nn.Parameter(p.clone().to(DEV)) for p in ps0]
    o_ref, o_got = make_ref(ref), make_got(got)
    other = Adam([torch.nn.Parameter(torch.zeros(3).to(DEV))])
    guard = _attach(other, o_got, None, clip)
    for step in range(3):
        for i, (a, b) in enumerate(zip(ref, got)):
            if i == 3:
                a.grad = b.grad = None                         # a frozen parameter
                continue
            g = _rnd(200 + 10 * step + i, *a.shape) * (0.1 if step == 2 else 1.0)
            a.grad, b.grad = g.clone(), g.to(DEV)
        total = torch.nn.utils.clip_grad_norm_(ref, clip)
        o_ref.step()
        o_got.step()
        row = guard.read()['G']
        print('step %d: torch norm %.9g, device norm %.9g coef %.9g' % (step, float(total), row['norm'], row['coef']))
        assert abs(row['norm'] - float(total)) <= 4e-6 * float(total) and row['skip'] == 0
        assert (row['coef'] < 1.0) == (float(total) + 1e-6 > clip)
        for a, b in zip(ref, got):
            TE.close(b, a, rtol=rtol, atol=atol)
    assert guard.counters()['G'] == {'steps': 3, 'skipped': 0, 'clipped': 2}    # (the third step's gradients are small)
    TE.close(o_got.state[got[1]][state_key], o_ref.state[ref[1]][state_key], rtol=rtol, atol=atol)
    return o_got


def test_clipped_adam_matches_torch():
    """optim.Adam under a guard with C = 30 (the norms of the three steps are about 66, 66 and 6.6) against
    torch.optim.Adam preceded by clip_grad_norm_ on CPU copies: test_adam_matches_torch's bounds (rtol 1e-6, atol 1e-7 of the
    tensor's scale), three steps, ragged shapes, one frozen parameter. (torch float32 against torch float64 on these inputs
    stays inside the bounds: a tenth of them at most, measured on the CPU.)"""
    from txt2vid_amd.optim import Adam
    opt = _clipped_against_torch(lambda ps: torch.optim.Adam(ps, lr=LR, betas=(B1, B2)), lambda ps: Adam(ps, lr=LR, betas=(B1, B2)),
                                 30.0, 1e-6, 1e-7, 'exp_avg')
    assert opt.step_dev is not None and opt.step_dev[0].item() == 3.0


@pytest.mark.parametrize('momentum', [0.0, 0.5])
def test_clipped_sgd_matches_torch(momentum):
    """The same for optim.SGD (test_sgd_matches_torch's bounds: rtol 1e-6, atol 1e-6)."""
    from txt2vid_amd.optim import SGD
    ps0 = [_rnd(100 + i, *sh) for i, sh in enumerate(SHAPES)]
    ref = [torch.nn.Parameter(p.clone()) for p in ps0]
    got = [torch.nn.Parameter(p.clone().to(DEV)) for p in ps0]
    o_ref, o_got = torch.optim.SGD(ref, lr=0.05, momentum=momentum), SGD(got, lr=0.05, momentum=momentum)
    guard = _attach(SGD([torch.nn.Parameter(torch.zeros(3).to(DEV))], lr=0.1), o_got, None, 30.0)
    for step in range(3):
        for i, (a, b) in enumerate(zip(ref, got)):
            if i == 3 and step == 1:
                a.grad = b.grad = None
                continue
            g = _rnd(200 + 10 * step + i, *a.shape)
            a.grad, b.grad = g.clone(), g.to(DEV)
        torch.nn.utils.clip_grad_norm_(ref, 30.0)
        o_ref.step()
        o_got.step()
        for a, b in zip(ref, got):
            TE.close(b, a, rtol=1e-6, atol=1e-6)
    assert guard.counters()['G'] == {'steps': 3, 'skipped': 0, 'clipped': 3}
    if momentum:
        TE.close(o_got.state[got[1]]['momentum_buffer'], o_ref.state[ref[1]]['momentum_buffer'], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize('momentum', [0.0, 0.5])
def test_sgd_skips_its_first_step_without_leaving_anything_uninitialised(momentum):
    from txt2vid_amd.optim import SGD
    p = torch.nn.Parameter(_rnd(1, 5000).to(DEV))
    twin = torch.nn.Parameter(p.detach().clone())
    opt, o_twin = SGD([p], lr=0.05, momentum=momentum), SGD([twin], lr=0.05, momentum=momentum)
    guard = _attach(opt, o_twin)
    before = _bits(p)
    p.grad = _rnd(2, 5000).to(DEV)
    p.grad[4999] = float('nan')
    opt.step()
    assert torch.equal(_bits(p), before) and guard.counters()['D'] == {'steps': 1, 'skipped': 1, 'clipped': 0}
    if momentum:
        assert not bool(opt.state[p]['momentum_buffer'].any())                     # zeros, not whatever the allocator held
    p.grad = _rnd(3, 5000).to(DEV)
    twin.grad = p.grad.clone()
    opt.step()
    o_twin.step()
    assert torch.equal(_bits(p), _bits(twin)) and not torch.equal(_bits(p), before)
    if momentum:
        assert torch.equal(opt.state[p]['momentum_buffer'], o_twin.state[twin]['momentum_buffer'])


class _Stack(torch.nn.Module):
    def __init__(self, sizes):
        super().__init__()
        self.layers = torch.nn.ModuleList([torch.nn.Linear(k, m) for m, k in sizes])


def test_spectral_norm_composes():
    """--D_sn: with a SpectralNorm hook attached, a step whose gradient holds a NaN leaves the master weights and the Adam state
    bitwise unchanged (the hook's projection and refresh run around it as always); a following finite step moves them."""
    from txt2vid_amd.gan.spectral import SpectralNorm
    from txt2vid_amd.optim import Adam
    torch.manual_seed(11)
    net = _Stack([(3 + i % 7, 20 + 13 * i) for i in range(6)]).to(DEV)
    sn = SpectralNorm([net], n_init=1, seed=5)
    opt = Adam(list(net.parameters()), lr=1e-2, betas=(B1, B2))
    opt.weight_hook = sn
    guard = _attach(opt, Adam([torch.nn.Parameter(torch.zeros(3).to(DEV))]))

    def step(seed, poison=False):
        gen = torch.Generator().manual_seed(seed)
        for p in net.parameters():
            p.grad = torch.randn(p.shape, generator=gen).to(DEV)
        if poison:
            net.layers[3].weight.grad[-1, -1] = float('nan')
        opt.step()
        torch.cuda.synchronize()

    def snap():
        return ([_bits(w) for w in sn.orig] + [_bits(l.bias) for l in net.layers] +
                [_bits(st[k]) for st in opt.state.values() for k in ('exp_avg', 'exp_avg_sq')] + [_bits(opt.step_dev)])
    step(1)
    s1 = snap()
    step(2, poison=True)
    s2 = snap()
    assert guard.counters()['D'] == {'steps': 2, 'skipped': 1, 'clipped': 0}
    assert len(s1) == 6 + 6 + 24 + 1 and all(torch.equal(a, b) for a, b in zip(s1, s2))
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
    step(3)
    s3 = snap()
    assert not any(torch.equal(a, b) for a, b in zip(s2, s3))
    assert guard.counters()['D'] == {'steps': 3, 'skipped': 1, 'clipped': 0} and opt.step_dev[0].item() == 2.0


# ------------------------------------------------------------------------------------------------ iteration level
NEW = ('t2v_grad_sumsq_multi', 't2v_grad_guard', 't2v_adam_tick_guard', 't2v_adam_multi_guard', 't2v_sgd_multi_guard')
OLD = ('t2v_adam_multi', 't2v_sgd_multi', 't2v_adam_tick')
NO_JOBS = ('t2v_grad_guard', 't2v_adam_tick_guard', 't2v_adam_tick')


def _counted(run):
    """`run()` with counting wrappers around the entry points: name -> the list of each call's job count (0 where there is none)."""
    from txt2vid_amd import functional as TF
    l = TF.lib()
    orig = {n: getattr(l, n) for n in NEW + OLD}
    calls = {n: [] for n in NEW + OLD}

    def wrap(n):
        def f(*a):
            calls[n].append(0 if n in NO_JOBS else int(a[1]))
            return orig[n](*a)
        return f
    try:
        for n in orig:
            setattr(l, n, wrap(n))
        out = run()
    finally:
        for n in orig:
            setattr(l, n, orig[n])
    return calls, out


def make(clips=None):
    """test_ema_gpu's B=4 set-up; `clips`: None (flags off) or (clip_D, clip_G), each a bound or None. A guard keeps Adam's step
    counter on the device from the first iteration on (`make_capturable` at attach time); the flag-off twin does the same by
    hand, so that both runs take their bias corrections from `t2v_adam_tick`'s float betas in every iteration — the host-side
    corrections of an eager iteration without the device counter come from the double betas and differ in the last bits."""
    gan, optD, optG, losses, prm = TE.make()
    guard = _attach(optD, optG, *clips) if clips is not None else None
    if guard is None:
        optD.make_capturable(DEV)
        optG.make_capturable(DEV)
    return gan, optD, optG, losses, prm, guard


def _params(gan):
    return {'G.' + k: _bits(p) for k, p in gan.gen.named_parameters()} | \
           {'D.' + k: _bits(p) for k, p in gan.discrims[0].named_parameters()}


def _moments(opts):
    return [_bits(st[k]) for opt in opts for st in opt.state.values() if st for k in ('exp_avg', 'exp_avg_sq')]


def _four_iterations(clips):
    """Four iterations (two eager, the capture + replay, one more replay) from seeds 100, under the counting wrappers; the guard's
    states read after every iteration."""
    from txt2vid_amd.gan.trainer import GraphedTrainStep
    gan, optD, optG, losses, prm, guard = make(clips)
    TE.seed(100)
    gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (4, 1, 16, 64, 64), warmup=2)
    rows = []

    def run():
        for x in TL.batches(4):
            gs.step(x)
            if guard is not None:
                rows.append(guard.read())
    calls, _ = _counted(run)
    assert gs.graphs is not None
    out = {'calls': calls, 'rows': rows, 'params': _params(gan), 'guard': guard}
    gs.release()
    return out


@pytest.fixture(scope='module')
def runs():
    """Flags off; --D_clip 1e30 --G_clip 1e30 (which also measures); then both bounds at half the norms the second run reported
    at its iteration 1."""
    off = _four_iterations(None)
    wide = _four_iterations((1e30, 1e30))
    half = (0.5 * wide['rows'][0]['D']['norm'], 0.5 * wide['rows'][0]['G']['norm'])
    bite = _four_iterations(half)
    return {'off': off, 'wide': wide, 'bite': bite, 'half': half}


def test_clipping_that_does_not_bite_changes_no_bit(runs):
    off, wide = runs['off'], runs['wide']
    assert len(off['params']) > 20 and off['params'].keys() == wide['params'].keys()
    for k in off['params']:
        assert torch.equal(off['params'][k], wide['params'][k]), k
    for i, r in enumerate(wide['rows'], start=1):
        print('iteration %d: %s' % (i, r))
        for w in ('D', 'G'):
            assert r[w]['coef'] == 1.0 and r[w]['skip'] == 0 and np.isfinite(r[w]['norm']) and r[w]['norm'] > 0
            assert (r[w]['steps'], r[w]['skipped'], r[w]['clipped']) == (i, 0, 0)


def test_clipping_that_bites(runs):
    wide, bite, half = runs['wide'], runs['bite'], runs['half']
    r = bite['rows'][0]
    print('bounds %s; iteration 1: %s' % (half, r))
    assert r['D']['norm'] == wide['rows'][0]['D']['norm']               # the same first gradients, bit for bit
    assert r['G']['norm'] != wide['rows'][0]['G']['norm']               # (G's come from a D that took a clipped step)
    for w, c in zip(('D', 'G'), half):
        assert r[w]['coef'] < 1.0 and G.within_one_ulp(r[w]['coef'], G.coef32(r[w]['norm'], c)) and r[w]['clipped'] == 1
    last = bite['rows'][-1]
    assert last['D']['clipped'] >= 1 and last['G']['clipped'] >= 1 and last['D']['steps'] == 4 and last['D']['skipped'] == 0
    differ = [k for k in wide['params'] if not torch.equal(wide['params'][k], bite['params'][k])]
    print('%d of %d tensors differ from the unclipped run' % (len(differ), len(wide['params'])))
    assert len(differ) > 20


def test_off_means_off(runs):
    """Flags off: none of the new entry points is called. Flags on: per optimiser step one sumsq call over exactly the jobs of the
    update launches (ceil(jobs / 64) launches), one decision, one guarded tick, the guarded update with the job lists the
    unguarded form got, and no unguarded update or tick. (Three Python passes: two eager iterations and the capture.)"""
    off, on = runs['off']['calls'], runs['wide']['calls']
    assert all(off[n] == [] for n in NEW), off
    unguarded = off['t2v_adam_multi']
    print('jobs per optimiser step:', unguarded)
    assert len(unguarded) == 6 and off['t2v_sgd_multi'] == [] and off['t2v_adam_tick'] == [0] * 6
    assert on['t2v_adam_multi_guard'] == unguarded
    assert on['t2v_grad_sumsq_multi'] == unguarded                     # one update launch group per step: the same job lists
    assert on['t2v_grad_guard'] == [0] * 6 and on['t2v_adam_tick_guard'] == [0] * 6
    assert on['t2v_adam_multi'] == [] and on['t2v_sgd_multi'] == [] and on['t2v_sgd_multi_guard'] == [] and on['t2v_adam_tick'] == []


# The NaN voxel of the bad batch. Both lie on the 8x8 level, which reads every eighth row and column of every sample and frame.
# D's stem is conv3 -> ReLU -> conv3 -> AvgPool((1, 2, 2), stride 2) on the residual path and that pooling -> conv1 on the skip
# path, and the pooling's frame stride keeps the even frames only:
#   frame 6: the skip path, which has no ReLU anywhere in D, carries the NaN to D's output: both losses, D's and G's gradients;
#   frame 7: the skip path never reads it, and the residual path's ReLU is fmaxf(x, 0), which maps NaN to 0, so D's outputs and
#            both losses stay finite; the NaN still enters the first convolution's weight gradient (0 * NaN) and only D is hit.
VOXELS = {'skip_path': (2, 0, 6, 24, 16), 'relu_path': (2, 0, 7, 24, 16)}


@pytest.fixture(scope='module', params=sorted(VOXELS))
def replayed(request):
    """--grad_guard on the small model: five finite iterations (two eager, the capture and two more replays), one replay whose
    clip holds a NaN voxel, one more finite replay; everything cloned around the bad one."""
    from txt2vid_amd.gan.trainer import GraphedTrainStep
    gan, optD, optG, losses, prm, guard = make((None, None))
    TE.seed(100)
    gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (4, 1, 16, 64, 64), warmup=2)
    xs = TL.batches(7)
    snaps = {}

    def snap(i):
        snaps[i] = {'params': _params(gan), 'mD': _moments((optD,)), 'mG': _moments((optG,)), 'rows': guard.read(),
                    'step_dev': {'D': _bits(optD.step_dev), 'G': _bits(optG.step_dev)}}
    for i, x in enumerate(xs[:5], start=1):
        gs.step(x)
    assert gs.graphs is not None and gs.n == 5
    snap(5)
    bad = xs[5].clone()
    bad[VOXELS[request.param]] = float('nan')
    lD, lG = gs.step(bad)
    snaps['losses'] = (float(lD), float(lG))
    snap(6)
    gs.step(xs[6])
    snap(7)
    return {'snaps': snaps, 'gs': gs, 'guard': guard, 'parts': (gan, optD, optG, losses, prm), 'voxel': request.param}


def _skipped_side(replayed, w):
    """Optimiser `w` skipped iteration 6 and nothing of it moved; iteration 7 moved everything that has a gradient."""
    s5, s6, s7 = (replayed['snaps'][i] for i in (5, 6, 7))
    assert (s5['rows'][w]['steps'], s5['rows'][w]['skipped']) == (5, 0)
    assert s6['rows'][w]['skip'] == 1 and not np.isfinite(s6['rows'][w]['norm']) and s6['rows'][w]['coef'] == 1.0
    assert (s6['rows'][w]['steps'], s6['rows'][w]['skipped'], s6['rows'][w]['clipped']) == (6, 1, 0)
    assert s7['rows'][w]['skip'] == 0 and np.isfinite(s7['rows'][w]['norm'])
    assert (s7['rows'][w]['steps'], s7['rows'][w]['skipped']) == (7, 1)
    names = [k for k in s5['params'] if k.startswith(w + '.')]
    m5, m6, m7 = (s['m' + w] for s in (s5, s6, s7))
    assert len(names) > 10 and len(m5) > 20
    for k in names:
        assert torch.equal(s6['params'][k], s5['params'][k]), k
    assert all(torch.equal(a, b) for a, b in zip(m5, m6))
    a, b, c = (s['step_dev'][w] for s in (s5, s6, s7))
    assert torch.equal(a, b) and a.view(torch.float32)[0].item() == 5.0 and c.view(torch.float32)[0].item() == 6.0
    # the next finite batch moves everything that has a gradient (all but structurally gradient-free tensors)
    live = [j for j in range(0, len(m5), 2) if bool(m5[j].any())]
    assert len(live) > 10
    for j in live:
        assert not torch.equal(m7[j], m6[j]) and not torch.equal(m7[j + 1], m6[j + 1]), j
    moved = [k for k in names if not torch.equal(s7['params'][k], s6['params'][k])]
    assert len(moved) >= len(live)
    assert all(bool(torch.isfinite(s7['params'][k].view(torch.float32)).all()) for k in names)


def test_the_decision_is_taken_at_replay_time(replayed):
    """The replay of a batch with one NaN voxel, by a graph captured three iterations earlier on finite data.
    A voxel the skip path reads (`VOXELS`): both losses are non-finite, BOTH steps are skipped — every parameter and moment of G
    and D and both device step counters bitwise unchanged, both `skipped` counts 1 — and the next finite batch moves them all.
    A voxel only the ReLU path reads: this build's ReLU drops the NaN from the forward pass, so the losses are finite (recorded
    on an MI355X: lossD 0.2904, lossG 3.4506) and G's gradients are too (norm 42.47): D's step is skipped in the same way, and
    G's, rightly, is taken."""
    s5, s6, s7 = (replayed['snaps'][i] for i in (5, 6, 7))
    print('%s: losses of the bad iteration %s; states %s' % (replayed['voxel'], replayed['snaps']['losses'], s6['rows']))
    _skipped_side(replayed, 'D')
    if replayed['voxel'] == 'skip_path':
        assert not any(np.isfinite(v) for v in replayed['snaps']['losses'])
        _skipped_side(replayed, 'G')
        assert s6['rows']['D']['skipped'] == 1 and s6['rows']['G']['skipped'] == 1
    else:
        assert all(np.isfinite(v) for v in replayed['snaps']['losses'])
        g = s6['rows']['G']
        assert g['skip'] == 0 and np.isfinite(g['norm']) and (g['steps'], g['skipped']) == (6, 0)
        assert s6['step_dev']['G'].view(torch.float32)[0].item() == 6.0
        moved = [k for k in s5['params'] if k.startswith('G.') and not torch.equal(s6['params'][k], s5['params'][k])]
        assert len(moved) > 10


def test_recapture_keeps_addresses_and_counts(replayed):
    """Another batch shape: a new GraphedTrainStep around the same optimisers counts on in the same device memory, and Adam's
    device step counter (for D 6 updates behind 7 steps, one skipped) stays authoritative."""
    from txt2vid_amd.gan.trainer import GraphedTrainStep
    gan, optD, optG, losses, prm = replayed['parts']
    guard = replayed['guard']
    was = guard.counters()
    assert was['D'] == {'steps': 7, 'skipped': 1, 'clipped': 0} and was['G']['steps'] == 7
    dev_was = (optD.step_dev[0].item(), optG.step_dev[0].item())
    assert dev_was == (7.0 - was['D']['skipped'], 7.0 - was['G']['skipped'])
    ptrs = [guard.state[w].data_ptr() for w in ('D', 'G')] + [optD.step_dev.data_ptr(), optG.step_dev.data_ptr(),
                                                              optD.grad_guard.partials.data_ptr()]
    replayed['gs'].release()
    gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (2, 1, 16, 64, 64), warmup=2)
    for i, x in enumerate(TL.batches(3, B=2, seed=12), start=8):
        gs.step(x)
        c = guard.counters()
        assert c['D'] == dict(was['D'], steps=i) and c['G'] == dict(was['G'], steps=i)
    assert gs.graphs is not None
    assert ptrs == [guard.state[w].data_ptr() for w in ('D', 'G')] + [optD.step_dev.data_ptr(), optG.step_dev.data_ptr(),
                                                                      optD.grad_guard.partials.data_ptr()]
    assert optD.grad_guard.state is guard.state['D'] and optG.grad_guard.state is guard.state['G']
    assert (optD.step_dev[0].item(), optG.step_dev[0].item()) == (dev_was[0] + 3.0, dev_was[1] + 3.0)
    assert optD.state_dict()['state'][0]['step'] == int(dev_was[0]) + 3
    gs.release()


# ------------------------------------------------------------------------------------------------ command line
def test_cli_round_trip(tmp_path):
    cfg = str(tmp_path / 'synth.json')
    with open(cfg, 'w') as f:
        json.dump({'class': 'txt2vid.data.my_dataset', 'args': {'data': 'synthetic', 'num_frames': 16, 'length': 64}}, f)
    base = ['--data', cfg, '--num_channels', '1', '--cuda', '--frame_sizes', '8', '16', '32', '64', '--D_names', 'video',
            '--G_lr', '0.0002', '--D_lr', '0.0004', '--D_beta1', '0.5', '--D_beta2', '.999', '--G_beta1', '0.5', '--G_beta2', '.999',
            '--D_loss', 'txt2vid.gan.losses.RSGANLoss', '--init_method', 'xavier', '--discrim_steps', '1', '--seed', '100',
            '--gp_lambda', '.5', '--subsample_input', '--workers', '0', '--log_period', '1', '--save_example_period', '0',
            '--G', 'txt2vid.models.tganv2.gen.MultiScaleGen', '--D', 'txt2vid.models.tganv2.discrim.MultiScaleDiscrim',
            '--dont_use_sent', '--batch_size', '8', '--epochs', '1']
    flags = ['--D_clip', '1e-3', '--G_clip', '1e30']

    def run(args):
        p = subprocess.run([sys.executable, '-m', 'txt2vid_amd.train.gan'] + base + args, cwd=ROOT, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=600)
        out = p.stdout.decode(errors='replace')
        assert p.returncode == 0, out[-3000:]
        return out

    def lines(log):
        """{loop iteration: (norm D, norm G, coef D, coef G, skipped D, skipped G, clipped D, clipped G)} from the log."""
        pat = (r'Iter (\d+), gradient guard: norm D (\S+) G (\S+), coef D (\S+) G (\S+), skipped D (\d+) G (\d+), '
               r'clipped D (\d+) G (\d+)')
        return {int(m[0]): tuple(float(v) for v in m[1:5]) + tuple(int(v) for v in m[5:]) for m in re.findall(pat, log)}
    out1 = str(tmp_path / 'out1')
    log = run(['--out', out1, '--out_samples', str(tmp_path / 's1'), '--max_iters', '4', '--save_model_period', '4'] + flags)
    assert 'Gradient guard: D clip 0.001, G clip 1e+30' in log and 'D 0 steps (0 skipped, 0 clipped)' in log, log[-3000:]
    got = lines(log)
    # under replay the values travel with the losses, one iteration late: the line of iteration i shows iteration i - 1
    assert sorted(got) == [2, 3, 4], log[-3000:]
    for i in (2, 3, 4):
        nD, nG, cD, cG, sD, sG, kD, kG = got[i]
        assert nD > 1e-3 and nG > 0 and 0 < cD < 1 and cG == 1.0 and (sD, sG, kG) == (0, 0, 0) and kD == i - 1, got
        assert abs(cD - 1e-3 / (nD + 1e-6)) <= 2e-5 * cD      # (both printed with six digits)
    ck = glob.glob(os.path.join(out1, 'iter_4_lossG_*'))
    assert len(ck) == 1
    sd = torch.load(ck[0], map_location='cpu', weights_only=False)
    assert sd['grad_guard'] == {'D': {'steps': 4, 'skipped': 0, 'clipped': 4}, 'G': {'steps': 4, 'skipped': 0, 'clipped': 0},
                                'config': {'clip_D': 1e-3, 'clip_G': 1e30}}
    # resume: the counts continue
    out2 = str(tmp_path / 'out2')
    log = run(['--out', out2, '--out_samples', str(tmp_path / 's2'), '--weights', ck[0], '--max_iters', '2', '--save_model_period', '2']
              + flags)
    assert 'D 4 steps (0 skipped, 4 clipped), G 4 steps (0 skipped, 0 clipped)' in log and 'no grad_guard key' not in log
    assert lines(log)[2][6] == 5
    ck2 = glob.glob(os.path.join(out2, 'iter_2_lossG_*'))
    assert len(ck2) == 1
    sd2 = torch.load(ck2[0], map_location='cpu', weights_only=False)
    assert sd2['grad_guard']['D'] == {'steps': 6, 'skipped': 0, 'clipped': 6} and sd2['grad_guard']['G']['steps'] == 6
    # the same file without the key: from zero, and it says so (eager launches: the values are read at the log period)
    bare = str(tmp_path / 'bare.pt')
    torch.save({k: v for k, v in sd.items() if k != 'grad_guard'}, bare)
    log = run(['--out', str(tmp_path / 'out3'), '--out_samples', str(tmp_path / 's3'), '--weights', bare, '--max_iters', '2',
               '--save_model_period', '0', '--no_graph', '--grad_guard'])
    assert 'no grad_guard key' in log and 'D 0 steps (0 skipped, 0 clipped)' in log and 'D clip off, G clip off' in log
    got = lines(log)
    assert sorted(got) == [1, 2] and got[2][2:] == (1.0, 1.0, 0, 0, 0, 0)
