"""GPU: the opt-in averaged generator (--G_ema) —
  (1) the three entry points against float64 at the derived fp32 bound, the gate, the swap, the refusals;
  (2) the recurrence over a real graph-replayed run, dead ConvLSTM taps, the --gen_steps schedule;
  (3) off means off: no call without an average, a fixed number with one;
  (4) `swapped()` really makes every kernel run the averaged weights (packed copies included) and restores bit for bit;
  (5) the command line: checkpoint keys, resume, sampling."""
import glob
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import tganv2_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24


def _jobs(pairs):
    from txt2vid_amd._lib import EmaJob
    arr = (EmaJob * len(pairs))()
    for a, (e, p) in zip(arr, pairs):
        a.e, a.p, a.n = e.data_ptr(), p.data_ptr(), e.numel()
    return arr


def _ema(pairs, d, start=0.0, count_dev=None, count_host=1.0):
    from txt2vid_amd import functional as TF
    st = TF.lib().t2v_ema_multi(_jobs(pairs), len(pairs), d, start, TF._p(count_dev), count_host, TF._stream())
    torch.cuda.synchronize()
    return st


def _rand(gen, n, off=0):
    """n fp32 values on the device, `off` elements into a 16-byte aligned buffer (off = 1: the unaligned scalar path)."""
    t = torch.randn(n + off, generator=gen).to(DEV)[off:]
    assert (t.data_ptr() % 16 == 0) == (off % 4 == 0)
    return t


# ------------------------------------------------------------------------------------------------ 1. op level
@pytest.mark.parametrize('d', [0.0, 0.5, 0.999])
def test_update_against_float64(d):
    """e = d e + (1 - d) p against float64. Bound (derived): three fp32 roundings — the two products and the sum, or the fused
    form — plus the rounding of 1 - d, each at most 2^-24 relative to max(|e|, |p|): |delta| <= 4 * 2^-24 * max(|e|, |p|)."""
    g = torch.Generator()
    g.manual_seed(17)
    pairs = [(_rand(g, n), _rand(g, n)) for n in (1, 4095, 4096, 4097, 1000003)]
    pairs.append((_rand(g, 5001, off=1), _rand(g, 5001, off=1)))
    e0 = [e.double().cpu() for e, _ in pairs]
    assert _ema(pairs, d) == 0
    for (e, p), old in zip(pairs, e0):
        pd = p.double().cpu()
        want = d * old + (1.0 - d) * pd
        bound = 4 * EPS * torch.maximum(old.abs(), pd.abs())
        err = (e.double().cpu() - want).abs()
        print('d=%g n=%d: max |delta| / bound = %.3f' % (d, e.numel(), float((err / bound.clamp_min(1e-300)).max())))
        assert bool((err <= bound).all()), (d, e.numel(), float(err.max()))
        if d == 0.0:
            assert torch.equal(e, p)


@pytest.mark.parametrize('d', [0.0, 0.5, 0.999])
def test_update_seventy_jobs_in_one_call(d):
    """More jobs than one launch holds (64): every one of them is updated, none twice."""
    g = torch.Generator()
    g.manual_seed(23)
    pairs = [(_rand(g, 100 + 61 * i), _rand(g, 100 + 61 * i)) for i in range(70)]
    e0 = [e.double().cpu() for e, _ in pairs]
    assert _ema(pairs, d) == 0
    for (e, p), old in zip(pairs, e0):
        pd = p.double().cpu()
        err = (e.double().cpu() - (d * old + (1.0 - d) * pd)).abs()
        assert bool((err <= 4 * EPS * torch.maximum(old.abs(), pd.abs())).all()), (d, e.numel())
        if d == 0.0:
            assert torch.equal(e, p)


@pytest.mark.parametrize('through', ['count_dev', 'count_host'])
def test_gate(through):
    """start = 3: an update count of 3 still copies, a count of 4 averages — read from the device or passed by the host."""
    g = torch.Generator()
    g.manual_seed(29)
    for count, averages in ((3.0, False), (4.0, True)):
        e, p = _rand(g, 10000), _rand(g, 10000)
        old = e.clone()
        dev = torch.tensor([count], device=DEV) if through == 'count_dev' else None
        assert _ema([(e, p)], 0.5, start=3.0, count_dev=dev, count_host=count if dev is None else -100.0) == 0
        if averages:
            want = 0.5 * old.double() + 0.5 * p.double()
            assert bool(((e.double() - want).abs() <= 4 * EPS * torch.maximum(old.abs(), p.abs()).double()).all())
            assert not torch.equal(e, p)
        else:
            assert torch.equal(e, p)


def test_tick_advances_the_device_count():
    from txt2vid_amd import functional as TF
    c = torch.tensor([41.0], device=DEV)
    for _ in range(3):
        assert TF.lib().t2v_ema_tick(TF._p(c), TF._stream()) == 0
    assert float(c[0]) == 44.0


def test_swap_twice_restores_both_sides_bitwise():
    from txt2vid_amd import functional as TF
    g = torch.Generator()
    g.manual_seed(31)
    pairs = [(_rand(g, n), _rand(g, n)) for n in (1, 4095, 4097, 300001)] + [(_rand(g, 777, off=1), _rand(g, 777, off=1))]
    pairs += [(_rand(g, 50 + i), _rand(g, 50 + i)) for i in range(66)]
    before = [(e.clone(), p.clone()) for e, p in pairs]
    arr = _jobs(pairs)
    assert TF.lib().t2v_swap_multi(arr, len(pairs), TF._stream()) == 0
    for (e, p), (e0, p0) in zip(pairs, before):
        assert torch.equal(e, p0) and torch.equal(p, e0)
    assert TF.lib().t2v_swap_multi(arr, len(pairs), TF._stream()) == 0
    for (e, p), (e0, p0) in zip(pairs, before):
        assert torch.equal(e, e0) and torch.equal(p, p0)


def test_refusals_return_without_launching():
    from txt2vid_amd import functional as TF
    from txt2vid_amd._lib import EmaJob
    l = TF.lib()
    e, p = torch.ones(64, device=DEV), torch.zeros(64, device=DEV)

    def job(ep, pp, n):
        arr = (EmaJob * 1)()
        arr[0].e, arr[0].p, arr[0].n = ep, pp, n
        return arr
    for arr, n in ((job(None, p.data_ptr(), 64), 1), (job(e.data_ptr(), None, 64), 1), (job(e.data_ptr(), p.data_ptr(), 0), 1),
                   (job(e.data_ptr(), p.data_ptr(), 2 ** 31), 1), (job(e.data_ptr(), p.data_ptr(), 64), 0), (None, 1)):
        assert l.t2v_ema_multi(arr, n, 0.0, 0.0, None, 1.0, TF._stream()) == -1
        assert l.t2v_swap_multi(arr, n, TF._stream()) == -1
    assert l.t2v_ema_tick(None, TF._stream()) == -1
    torch.cuda.synchronize()
    assert bool((e == 1).all()) and bool((p == 0).all())


# ------------------------------------------------------------------------------------------------ helpers for the runs
def pour(module):
    module.load_state_dict({k: O.recipe_tensor(k, v.shape) for k, v in module.state_dict().items()})
    return module.to(DEV)


def make(decay=None, start=0, gen_steps=1, keyword=True):
    """B=4 unconditional 64x64 set-up of the step tests (recipe weights, RSGAN + GP 0.5, Adam). `decay=None`: no average;
    `keyword=False`: the CondGan is built without the gen_ema keyword at all."""
    from txt2vid_amd.models.tganv2.gen import MultiScaleGen
    from txt2vid_amd.models.tganv2.discrim import MultiScaleDiscrim
    from txt2vid_amd.gan.cond_gan import CondGan
    from txt2vid_amd.gan.ema import GenAverage
    from txt2vid_amd.gan.losses import MixedGanLoss, RSGANLoss
    from txt2vid_amd.optim import Adam
    gen = pour(MultiScaleGen(width=64, height=64, num_channels=1)).train()
    dis = pour(MultiScaleDiscrim(num_channels=1)).train()
    kw = {}
    if keyword:
        kw['gen_ema'] = GenAverage(gen, decay, start=start) if decay is not None else None
    gan = CondGan(gen=gen, discrims=[dis], discrim_names=['video'], **kw)
    losses = MixedGanLoss(g_loss=RSGANLoss(), d_loss=RSGANLoss())
    optD = Adam([{'params': dis.parameters()}], lr=2e-4, betas=(0.5, 0.999))
    optG = Adam([{'params': gen.parameters()}], lr=2e-4, betas=(0.5, 0.999))

    class Prm(object):
        frame_sizes = [8, 16, 32, 64]
        subsample_input = True
        discrim_steps = 1
        gp_lambda = 0.5
        no_mean_discrim_loss = no_mean_gen_loss = True
    Prm.gen_steps = gen_steps
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


@pytest.fixture(scope='module')
def trained():
    """Eight iterations (2 eager, capture + replay, 5 replays) with --G_ema 0.5 --G_ema_start 2, seeds 100; the generator's
    parameters and the averaged tensors cloned after every iteration."""
    from txt2vid_amd.gan.trainer import GraphedTrainStep
    gan, optD, optG, losses, prm = make(decay=0.5, start=2)
    init = {k: p.detach().clone() for k, p in gan.gen.named_parameters()}
    seed(100)
    gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (4, 1, 16, 64, 64), warmup=2)
    clones, averages = [], []
    for _ in range(8):
        gs.step(batch())
        torch.cuda.synchronize()
        clones.append({k: p.detach().clone() for k, p in gan.gen.named_parameters()})
        averages.append({k: e.clone() for k, e in gan.gen_ema.state_dict().items()})
    assert gs.graphs is not None
    return gan, gs, init, clones, averages


# ------------------------------------------------------------------------------------------------ 2. recurrence
def test_recurrence_over_a_graph_replayed_run(trained):
    """After iteration k the average equals the float64 recurrence over the cloned weights (copies while the count is <= 2,
    then e = 0.5 e + 0.5 p) within 2 * 4 * 2^-24 * max|p|: with d = 0.5 the per-step bound of the op test sums to at most
    twice itself (max|p| over the weights seen so far). Checked after every iteration: the two eager warm-up iterations, the
    captured one and the five replays."""
    gan, gs, init, clones, averages = trained
    assert gan.gen_ema.updates == 8
    worst = 0.0
    for k in averages[0]:
        ref, top = None, 0.0
        for t, (snap, avg) in enumerate(zip(clones, averages), start=1):
            p = snap[k].double()
            top = max(top, float(p.abs().max()))
            ref = p.clone() if t <= 2 else 0.5 * ref + 0.5 * p
            err = float((avg[k].double() - ref).abs().max())
            bound = 2 * 4 * EPS * top
            worst = max(worst, err / bound if bound > 0 else 0.0)
            assert err <= bound, (k, t, err, bound)
            if t <= 2:
                assert torch.equal(avg[k], snap[k]), (k, t)                     # before the start: a plain copy
        assert torch.equal(gan.gen_ema.state_dict()[k], averages[-1][k]), k
    print('recurrence: worst |delta| / bound = %.3f' % worst)


def test_dead_convlstm_taps_keep_the_initial_weights(trained):
    """Averaged dead ConvLSTM taps (and the weights' own) are `torch.equal` to the initial weights after the eight iterations."""
    from txt2vid_amd import functional as TF
    gan, gs, init, clones, averages = trained
    named = dict(gan.gen.named_parameters())
    sd = gan.gen_ema.state_dict()
    seen, bad = 0, []
    for k, p in named.items():
        live = getattr(p, '_t2v_live_taps', None)
        if live is None:
            continue
        seen += 1
        rows_e, rows_0, rows_p = TF.tap_rows(sd[k]), TF.tap_rows(init[k]), TF.tap_rows(p.detach())
        for t in range(rows_e.shape[0]):
            de, dp = float((rows_e[t] - rows_0[t]).abs().max()), float((rows_p[t] - rows_0[t]).abs().max())
            print('%s tap %d (%s): max |e - init| %.3e  max |p - init| %.3e' % (k, t, 'live' if t in live else 'dead', de, dp))
            if t in live:
                # live taps moved — except Wxf's: x enters at step 0 only, where the forget gate multiplies c_0 = 0, so its
                # gradient is exactly 0 and Adam leaves it where it is; no claim is made for that one
                if torch.equal(rows_e[t], rows_0[t]) and not k.endswith('Wxf.weight'):
                    bad.append((k, t, 'live tap did not move'))
            elif not (torch.equal(rows_e[t], rows_0[t]) and torch.equal(rows_p[t], rows_0[t])):
                bad.append((k, t, de, dp))
    assert seen == 8
    assert not bad, bad


def test_two_gen_steps_make_two_updates_per_iteration():
    from txt2vid_amd.gan.trainer import GraphedTrainStep
    gan, optD, optG, losses, prm = make(decay=0.5, start=2, gen_steps=2)
    seed(100)
    gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (4, 1, 16, 64, 64), warmup=2)
    for i in range(4):
        gs.step(batch())
        assert gan.gen_ema.updates == 2 * (i + 1)
    assert gs.graphs is not None
    assert gan.save_dict()['gen_ema_updates'] == 8


# ------------------------------------------------------------------------------------------------ 3. off means off
def _counted(run):
    """Run `run()` with counting wrappers around the three entry points of the loaded library."""
    from txt2vid_amd import functional as TF
    l = TF.lib()
    names = ('t2v_ema_multi', 't2v_ema_tick', 't2v_swap_multi')
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
    out = []
    for _ in range(3):
        lD, lG = gs.step(batch())
        out.append((float(lD), float(lG)))
    assert gs.graphs is not None
    return out


def test_off_means_off():
    """Without an average three iterations (two eager, one captured and replayed) call none of the new entry points; with one
    they make one tick and ceil(jobs / 64) update calls per generator update in each of the three Python passes (the replay
    itself makes none). The losses of the flag-off run are compared with a CondGan built without the keyword at all: nothing
    differs between the two, but tools/det_check.py has not recorded this path as run-to-run deterministic (the autograd
    accumulation order varies, see test_models_gpu.test_graph_replay_matches_eager), so the comparison is that test's for two
    runs of the same code: 5e-6 on the eager iterations, 5e-4 on the replayed one."""
    _three_iterations(*make(keyword=False))                        # burn-in (see test_graph_replay_matches_eager)
    calls, plain = _counted(lambda: _three_iterations(*make(keyword=False)))
    assert calls == {'t2v_ema_multi': 0, 't2v_ema_tick': 0, 't2v_swap_multi': 0}
    calls, off = _counted(lambda: _three_iterations(*make(decay=None)))
    assert calls == {'t2v_ema_multi': 0, 't2v_ema_tick': 0, 't2v_swap_multi': 0}
    for i, (a, b) in enumerate(zip(off, plain)):
        print('iteration %d: gen_ema=None %s | no keyword %s' % (i, a, b))
        tol = 5e-6 if i < 2 else 5e-4
        assert abs(a[0] - b[0]) < tol and abs(a[1] - b[1]) < tol, (i, a, b)
    parts = make(decay=0.999)
    calls, _ = _counted(lambda: _three_iterations(*parts))
    jobs = parts[0].gen_ema.n_jobs
    assert jobs == len(list(parts[0].gen.parameters()))            # one job per tensor, the live centre tap of the 8 ConvLSTM weights
    assert calls == {'t2v_ema_tick': 3, 't2v_ema_multi': 3 * ((jobs + 63) // 64), 't2v_swap_multi': 0}
    assert parts[0].gen_ema.updates == 3


# ------------------------------------------------------------------------------------------------ 4. swap
def test_swapped_runs_the_averaged_weights_and_restores(trained):
    """y_avg (inside `swapped()`) against a FRESH generator loaded with the averaged parameters: two runs of the same kernels on
    the same weights, compared like test_models_gpu.test_gen compares its eval video (rtol 2e-3, atol 5e-4 of the scale; that
    forward has not been recorded as bitwise deterministic). y_avg must differ from the live generator's output by more than
    that tolerance — the packed weight copies were really refreshed — and everything is restored bit for bit afterwards,
    also when the body raises."""
    from txt2vid_amd.models.tganv2.gen import MultiScaleGen
    gan, gs, init, clones, averages = trained
    gen, ema = gan.gen, gan.gen_ema
    g = torch.Generator()
    g.manual_seed(3)
    z = torch.randn(2, gen.latent_size, generator=g).to(DEV)
    gen.eval()
    try:
        with torch.no_grad():
            y_live = gen(z)[0].clone()
            before = {k: p.detach().clone() for k, p in gen.named_parameters()}
            avg_before = {k: e.clone() for k, e in ema.state_dict().items()}
            with ema.swapped():
                y_avg = gen(z)[0].clone()
                for k, p in gen.named_parameters():
                    assert torch.equal(p.detach(), avg_before[k]), k
            fresh = MultiScaleGen(width=64, height=64, num_channels=1)
            sd = {k: v.detach().clone() for k, v in gen.state_dict().items()}
            sd.update({k: v.detach().clone() for k, v in ema.state_dict().items()})
            fresh.load_state_dict(sd)
            fresh.to(DEV).eval()
            y_ref = fresh(z)[0]
            print('max |y_avg - y_ref| %.3e   max |y_avg - y_live| %.3e' % (float((y_avg - y_ref).abs().max()),
                                                                           float((y_avg - y_live).abs().max())))
            close(y_avg, y_ref, rtol=2e-3, atol=5e-4)
            with pytest.raises(AssertionError):
                close(y_avg, y_live, rtol=2e-3, atol=5e-4)
            for k, p in gen.named_parameters():
                assert torch.equal(p.detach(), before[k]), k
                assert torch.equal(ema.state_dict()[k], avg_before[k]), k
            close(gen(z)[0], y_live, rtol=2e-3, atol=5e-4)
            with pytest.raises(ZeroDivisionError):
                with ema.swapped():
                    1 / 0
            for k, p in gen.named_parameters():
                assert torch.equal(p.detach(), before[k]), k
                assert torch.equal(ema.state_dict()[k], avg_before[k]), k
            close(gen(z)[0], y_live, rtol=2e-3, atol=5e-4)
    finally:
        gen.train()


def test_swapped_refuses_stream_capture(trained, monkeypatch):
    """The guard is `torch.cuda.is_current_stream_capturing()`; it is made to answer True here instead of opening a capture that
    would then have to be torn down around the exception. Nothing is exchanged."""
    gan = trained[0]
    before = {k: p.detach().clone() for k, p in gan.gen.named_parameters()}
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    with pytest.raises(RuntimeError, match='stream capture'):
        with gan.gen_ema.swapped():
            pass
    monkeypatch.undo()
    for k, p in gan.gen.named_parameters():
        assert torch.equal(p.detach(), before[k]), k


# ------------------------------------------------------------------------------------------------ 5. command line
def test_cli_round_trip(tmp_path):
    cfg = str(tmp_path / 'synth.json')
    with open(cfg, 'w') as f:
        json.dump({'class': 'txt2vid.data.my_dataset', 'args': {'data': 'synthetic', 'num_frames': 16, 'length': 64}}, f)
    base = ['--data', cfg, '--num_channels', '1', '--cuda', '--frame_sizes', '8', '16', '32', '64', '--D_names', 'video',
            '--G_lr', '0.0002', '--D_lr', '0.0002', '--D_beta1', '0.5', '--D_beta2', '.999', '--G_beta1', '0.5', '--G_beta2', '.999',
            '--D_loss', 'txt2vid.gan.losses.RSGANLoss', '--init_method', 'xavier', '--discrim_steps', '1', '--seed', '100',
            '--gp_lambda', '.5', '--subsample_input', '--workers', '0', '--log_period', '1',
            '--G', 'txt2vid.models.tganv2.gen.MultiScaleGen', '--D', 'txt2vid.models.tganv2.discrim.MultiScaleDiscrim',
            '--dont_use_sent', '--batch_size', '8', '--epochs', '1']

    def run(args):
        p = subprocess.run([sys.executable, '-m', 'txt2vid_amd.train.gan'] + base + args, cwd=ROOT, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=600)
        out = p.stdout.decode(errors='replace')
        assert p.returncode == 0, out[-3000:]
        return out
    out1, smp1 = str(tmp_path / 'out1'), str(tmp_path / 'samples1')
    log = run(['--out', out1, '--out_samples', smp1, '--G_ema', '0.9', '--max_iters', '4', '--save_model_period', '4',
               '--save_example_period', '4'])
    assert 'Iter 4, Loss_D' in log and 'averaged generator' in log
    ck = glob.glob(os.path.join(out1, 'iter_4_lossG_*'))
    assert len(ck) == 1
    sd = torch.load(ck[0], map_location='cpu', weights_only=False)
    assert sd['gen_ema_updates'] == 4
    from txt2vid_amd.models.tganv2.gen import MultiScaleGen
    want = {k: tuple(p.shape) for k, p in MultiScaleGen(width=64, height=64, num_channels=1).named_parameters()}
    assert {k: tuple(v.shape) for k, v in sd['gen_ema'].items()} == want
    assert len(glob.glob(os.path.join(smp1, 'fake_samples_epoch_000_iter_000004_*.png'))) == 4
    assert os.path.exists(os.path.join(smp1, 'real_samples.png'))
    # resume for two more iterations: the count carries on and the average moves
    out2 = str(tmp_path / 'out2')
    log = run(['--out', out2, '--out_samples', str(tmp_path / 'samples2'), '--G_ema', '0.9', '--weights', ck[0], '--max_iters', '2',
               '--save_model_period', '2', '--save_example_period', '0'])
    assert '(4 updates so far)' in log
    ck2 = glob.glob(os.path.join(out2, 'iter_2_lossG_*'))
    assert len(ck2) == 1
    sd2 = torch.load(ck2[0], map_location='cpu', weights_only=False)
    assert sd2['gen_ema_updates'] == 6
    assert set(sd2['gen_ema']) == set(want)
    moved = [k for k in want if not torch.equal(sd2['gen_ema'][k], sd['gen_ema'][k])]
    assert 'fc.weight' in moved and 'render_blocks.3.conv.weight' in moved, moved
    # sampling: with the flag the averaged generator renders, without it the extra keys are ignored
    for flag, name in ((['--G_ema', '0.9'], 'test_avg'), ([], 'test_live')):
        smp = str(tmp_path / name)
        log = run(['--out', out2, '--out_samples', smp, '--test', '--weights', ck2[0], '--num_samples', '1', '--max_iters', '1'] + flag)
        assert os.path.exists(os.path.join(smp, 'real_0.png')) and os.path.exists(os.path.join(smp, '64x64_0_0.jpg'))
        assert ('averaged generator' in log) == bool(flag)
