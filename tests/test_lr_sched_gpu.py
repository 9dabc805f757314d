"""GPU: learning-rate decay inside the replayed graph (--lr_decay) —
  (4) the tick: 14 updates of the device state against float64, the ends bit-exact;
  (5) the scheduled multi-tensor launches are the existing ones called with the float product, bit for bit;
  (6) a replayed iteration reads the state: with a rate that reaches 0 the parameters stop, the moments do not;
  (7) a capture for another batch shape carries the counters on;
  (8) off means off;
  (9) the command line: checkpoint key, the logged rates, resume, a file without the key, other flags."""
import glob
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import lr_cases as L
import test_ema_gpu as TE                  # (its set-up helpers: make, seed)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND_ID = {'linear': 1, 'cosine': 2}
LR = 2e-4


def _state(k=0.0, factor=1.0):
    return torch.tensor([k, factor], dtype=torch.float32).to(DEV)


# ------------------------------------------------------------------------------------------------ 4. tick
@pytest.mark.parametrize('spi', [1, 2])
@pytest.mark.parametrize('kind', L.KINDS)
def test_tick_sequence(kind, spi):
    from txt2vid_amd import functional as TF
    st = _state()
    for i in range(1, 15):
        assert TF.lib().t2v_lr_tick(TF._p(st), KIND_ID[kind], L.S, L.T, L.F, spi, TF._stream()) == 0
        k, f = (np.float32(v) for v in st.tolist())
        it = (i - 1) // spi                                # the update just announced is update i - 1
        want = L.factor(kind, it)
        print('%s spi %d: tick %2d -> k %g, factor %.9g (float64 %.17g)' % (kind, spi, i, k, f, want))
        assert k == i
        assert L.within_one_ulp(f, want), (i, f, want)
        if it <= L.S:
            assert f == np.float32(1.0)
        if it >= L.T:
            assert f == np.float32(L.F)
        if L.S < it < L.T:
            assert np.float32(L.F) < f < np.float32(1.0)


# ------------------------------------------------------------------------------------------------ 5. scheduled = existing with the product
SIZES = (1, 3, 4095, 4096, 4097, 8193)


def _tensors(gen, n, off=0):
    """p, g, m, v of n elements, `off` floats into 16-byte aligned buffers (off = 1: the scalar path); v >= 0."""
    out = []
    for i in range(4):
        t = torch.randn(n + off, generator=gen)
        t = (t.abs() * 1e-3 if i == 3 else t).to(DEV)[off:]
        assert (t.data_ptr() % 16 == 0) == (off % 4 == 0)
        out.append(t)
    return tuple(out)


def _job_sets():
    """The seven-job call (the sizes around the 4096-element chunk, one job off alignment) and a 70-job call (two launches)."""
    gen = torch.Generator()
    gen.manual_seed(41)
    few = [_tensors(gen, n) for n in SIZES] + [_tensors(gen, 5001, off=1)]
    many = [_tensors(gen, 50 + 37 * i, off=(1 if i == 5 else 0)) for i in range(70)]
    return few, many


def _jobs(items, with_v=True):
    from txt2vid_amd._lib import AdamJob
    arr = (AdamJob * len(items))()
    for a, (p, g, m, v) in zip(arr, items):
        a.p, a.g, a.m, a.n = p.data_ptr(), g.data_ptr(), (m.data_ptr() if m is not None else None), p.numel()
        a.v = v.data_ptr() if with_v else None
    return arr


def _clone(items):
    """Copies with the alignment of the originals (a clone of an offset view would be aligned again)."""
    out = []
    for ts in items:
        off = (ts[0].data_ptr() % 16) // 4
        cs = []
        for t in ts:
            c = torch.empty(t.numel() + off, device=DEV, dtype=torch.float32)[off:]
            c.copy_(t)
            assert c.data_ptr() % 16 == t.data_ptr() % 16
            cs.append(c)
        out.append(tuple(cs))
    return out


@pytest.fixture(scope='module')
def job_sets():
    return _job_sets()


@pytest.mark.parametrize('with_step_dev', [False, True])
@pytest.mark.parametrize('factor', [1.0, 0.37, 0.0])
def test_scheduled_adam_is_adam_with_the_product(job_sets, factor, with_step_dev):
    """t2v_adam_multi_sched(lr, state) against t2v_adam_multi(float32(lr) * float32(factor)): p, m and v bit for bit."""
    from txt2vid_amd import functional as TF
    l = TF.lib()
    b1, b2, eps, step = 0.5, 0.999, 1e-8, 3
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    step_dev = torch.tensor([float(step), bc1, bc2], dtype=torch.float32).to(DEV) if with_step_dev else None
    host_bc = (7.0, 7.0) if with_step_dev else (bc1, bc2)          # (ignored when the device triple is given)
    product = float(np.float32(LR) * np.float32(factor))
    st = _state(9.0, factor)
    for items in job_sets:
        a, b = _clone(items), _clone(items)
        assert l.t2v_adam_multi_sched(_jobs(a), len(a), LR, TF._p(st), b1, b2, eps, host_bc[0], host_bc[1], 0.5, TF._p(step_dev),
                                      TF._stream()) == 0
        assert l.t2v_adam_multi(_jobs(b), len(b), product, b1, b2, eps, host_bc[0], host_bc[1], 0.5, TF._p(step_dev), TF._stream()) == 0
        torch.cuda.synchronize()
        assert st.tolist() == [9.0, float(np.float32(factor))]     # the launch only reads the state
        for (pa, ga, ma, va), (pb, gb, mb, vb), (p0, g0, m0, v0) in zip(a, b, items):
            n = p0.numel()
            assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb), (factor, n)
            assert torch.equal(ga, g0)
            assert not torch.equal(ma, m0) and not torch.equal(va, v0), n
            if factor == 0.0:
                assert torch.equal(pa.view(torch.int32), p0.view(torch.int32)), n      # the rate is 0: p bitwise unchanged
            else:
                assert not torch.equal(pa, p0), n


@pytest.mark.parametrize('first', [0, 1])
@pytest.mark.parametrize('mu', [0.0, 0.5])
def test_scheduled_sgd_is_sgd_with_the_product(job_sets, mu, first):
    from txt2vid_amd import functional as TF
    l = TF.lib()
    for factor in (1.0, 0.37, 0.0):
        product = float(np.float32(LR * 100) * np.float32(factor))
        st = _state(2.0, factor)
        for items in job_sets:
            a, b = _clone(items), _clone(items)
            assert l.t2v_sgd_multi_sched(_jobs(a, False), len(a), LR * 100, TF._p(st), mu, 0.5, first, TF._stream()) == 0
            assert l.t2v_sgd_multi(_jobs(b, False), len(b), product, mu, 0.5, first, TF._stream()) == 0
            torch.cuda.synchronize()
            for (pa, ga, ma, va), (pb, gb, mb, vb), (p0, g0, m0, v0) in zip(a, b, items):
                n = p0.numel()
                assert torch.equal(pa, pb) and torch.equal(ma, mb), (factor, mu, first, n)
                assert torch.equal(va, v0) and torch.equal(ga, g0)
                assert torch.equal(ma, m0) == (mu == 0.0), n                           # the buffer moves unless there is none
                if factor == 0.0:
                    assert torch.equal(pa.view(torch.int32), p0.view(torch.int32)), n
                else:
                    assert not torch.equal(pa, p0), n


# ------------------------------------------------------------------------------------------------ helpers for the runs
def batches(n, B=4, seed=11):
    g = torch.Generator()
    g.manual_seed(seed)
    return [(torch.rand(B, 1, 16, 64, 64, generator=g) * 2 - 1).to(DEV) for _ in range(n)]


def make(n_d=1, n_g=1, schedule=('linear', 5, 0, 0.0)):
    """test_ema_gpu's B=4 unconditional set-up under an N:M step schedule; `schedule`: (kind, T, S, F) or None."""
    from txt2vid_amd.gan.lr_sched import LrSchedule
    gan, optD, optG, losses, prm = TE.make(gen_steps=n_g)
    prm.discrim_steps = n_d
    sched = None
    if schedule is not None:
        kind, T, S, F = schedule
        sched = LrSchedule(kind, T, S, F, n_d, n_g, DEV).attach(optD, optG)
    return gan, optD, optG, losses, prm, sched


def _params(gan):
    return {'G.' + k: p.detach().clone() for k, p in gan.gen.named_parameters()} | \
           {'D.' + k: p.detach().clone() for k, p in gan.discrims[0].named_parameters()}


def _moments(opts):
    return [st['exp_avg'].clone() for opt in opts for st in opt.state.values() if st]


@pytest.fixture(scope='module', params=[(1, 1), (2, 1)], ids=['1to1', '2to1'])
def replayed(request):
    """--lr_decay linear --lr_decay_iters 5 --lr_final 0 on the small model: five eager-only iterations, then the same seeds
    through 2 eager iterations, the capture and 5 replays (7 iterations), with the state read after every one."""
    from txt2vid_amd.gan.trainer import train_iteration, GraphedTrainStep
    n_d, n_g = request.param
    gan, optD, optG, losses, prm, _ = make(n_d, n_g, None)
    train_iteration(gan, batches(1)[0], None, optD, optG, losses, prm, DEV)      # burn-in (see test_graph_replay_matches_eager)
    gan, optD, optG, losses, prm, sched = make(n_d, n_g)
    TE.seed(100)
    eager = []
    for x in batches(5):
        lD, lG, _, _ = train_iteration(gan, x, None, optD, optG, losses, prm, DEV)
        eager.append((float(lD), float(lG)))
    assert sched.counters() == {'D': 5 * n_d, 'G': 5 * n_g}
    gan, optD, optG, losses, prm, sched = make(n_d, n_g)
    TE.seed(100)
    gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (4, 1, 16, 64, 64), warmup=2)
    rec = {'losses': [], 'counters': [], 'params': {}, 'moments': {}, 'factors': []}
    for i, x in enumerate(batches(7), start=1):
        lD, lG = gs.step(x)
        rec['losses'].append((float(lD), float(lG)))
        rec['counters'].append(sched.counters())
        rec['factors'].append((float(sched.state['D'][1]), float(sched.state['G'][1])))
        if i >= 5:
            rec['params'][i] = _params(gan)
            rec['moments'][i] = _moments((optD, optG))
    assert gs.graphs is not None and gs.n == 7
    return {'n_d': n_d, 'n_g': n_g, 'eager': eager, 'rec': rec, 'gs': gs, 'sched': sched, 'parts': (gan, optD, optG, losses, prm)}


# ------------------------------------------------------------------------------------------------ 6. the replay reads the state
def test_replay_reads_the_state(replayed):
    """The factors are 1, .8, .6, .4, .2 and then 0: after iteration 5 the counters read 5 N and 5 M, and iterations 6 and 7 — both
    replays of a graph captured at iteration 3, when the factor was 0.6 — leave every parameter of G and D bitwise unchanged,
    while exp_avg keeps moving. A rate baked into the graph at capture time would keep moving them."""
    n_d, n_g, rec = replayed['n_d'], replayed['n_g'], replayed['rec']
    for i, c in enumerate(rec['counters'], start=1):
        assert c == {'D': i * n_d, 'G': i * n_g}, (i, c)
    for i, f in enumerate(rec['factors'], start=1):
        want = np.float32(L.factor('linear', i - 1, 0, 5, 0.0))
        print('iteration %d: factors on the device %r, float64 %.17g' % (i, f, want))
        assert L.within_one_ulp(f[0], want) and f[0] == f[1]
    assert rec['factors'][5] == (0.0, 0.0) and rec['factors'][6] == (0.0, 0.0)
    p5, p6, p7 = (rec['params'][i] for i in (5, 6, 7))
    assert len(p5) > 20
    for k in p5:
        assert torch.equal(p6[k].view(torch.int32), p5[k].view(torch.int32)), k
        assert torch.equal(p7[k].view(torch.int32), p5[k].view(torch.int32)), k
    m5, m6, m7 = (rec['moments'][i] for i in (5, 6, 7))
    live = [j for j, m in enumerate(m5) if bool((m != 0).any())]       # (all but gradient-free tensors, e.g. the ConvLSTM's Wxf)
    print('%d of %d exp_avg tensors are non-zero after iteration 5' % (len(live), len(m5)))
    assert len(live) > 20
    for j in live:
        assert not torch.equal(m6[j], m5[j]) and not torch.equal(m7[j], m6[j]), j


def test_first_five_iterations_match_the_eager_run(replayed):
    """test_graph_replay_matches_eager's bounds: 5e-6 on the eager iterations, 5e-4 on the replayed ones."""
    for i, (got, want) in enumerate(zip(replayed['rec']['losses'][:5], replayed['eager'])):
        print('iteration %d (%s): %s vs eager-only %s' % (i + 1, 'replay' if i >= 2 else 'eager', got, want))
    for i, (got, want) in enumerate(zip(replayed['rec']['losses'][:5], replayed['eager'])):
        tol = 5e-6 if i < 2 else 5e-4
        assert abs(got[0] - want[0]) < tol and abs(got[1] - want[1]) < tol, (i, got, want)


# ------------------------------------------------------------------------------------------------ 7. re-capture
def test_recapture_continues_the_counters(replayed):
    """Another batch shape (an epoch's short last batch): a new GraphedTrainStep around the same optimisers — `make_capturable`
    again, 2 eager iterations, a new capture — counts on from 7 N / 7 M in the same device memory."""
    from txt2vid_amd.gan.trainer import GraphedTrainStep
    n_d, n_g, sched = replayed['n_d'], replayed['n_g'], replayed['sched']
    gan, optD, optG, losses, prm = replayed['parts']
    ptrs = {w: t.data_ptr() for w, t in sched.state.items()}
    assert sched.counters() == {'D': 7 * n_d, 'G': 7 * n_g}
    replayed['gs'].release()
    gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (2, 1, 16, 64, 64), warmup=2)
    for i, x in enumerate(batches(3, B=2, seed=12), start=8):
        gs.step(x)
        assert sched.counters() == {'D': i * n_d, 'G': i * n_g}
    assert gs.graphs is not None
    assert {w: t.data_ptr() for w, t in sched.state.items()} == ptrs
    assert optD.lr_sched.state is sched.state['D'] and optG.lr_sched.state is sched.state['G']
    assert int(optD.step_dev[0].item()) == 10 * n_d and int(optG.step_dev[0].item()) == 10 * n_g
    assert optD.param_groups[0]['lr'] == LR and optG.param_groups[0]['lr'] == LR        # the base rates stay visible


# ------------------------------------------------------------------------------------------------ 8. off means off
NEW = ('t2v_lr_tick', 't2v_adam_multi_sched', 't2v_sgd_multi_sched')
OLD = ('t2v_adam_multi', 't2v_sgd_multi')


def _counted(run):
    """`run()` with counting wrappers around the entry points: name -> the list of each call's job count (0 for the tick)."""
    from txt2vid_amd import functional as TF
    l = TF.lib()
    orig = {n: getattr(l, n) for n in NEW + OLD}
    calls = {n: [] for n in NEW + OLD}

    def wrap(n):
        def f(*a):
            calls[n].append(0 if n == 't2v_lr_tick' else int(a[1]))
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


def _three_iterations(gan, optD, optG, losses, prm, sched, strip=False):
    from txt2vid_amd.gan.trainer import GraphedTrainStep
    if strip:                              # optimisers "built without the attribute at all"
        del optD.lr_sched, optG.lr_sched
        assert not hasattr(optD, 'lr_sched')
    TE.seed(100)
    gs = GraphedTrainStep(gan, optD, optG, losses, prm, DEV, (4, 1, 16, 64, 64), warmup=2)
    out = []
    for x in batches(3):
        lD, lG = gs.step(x)
        out.append((float(lD), float(lG)))
    assert gs.graphs is not None
    return out


def test_off_means_off():
    """Flag off: three iterations (two eager, one captured and replayed) call none of the new entry points, and their losses
    are those of optimisers without the attribute at all (test_ema_gpu.test_off_means_off's bounds: 5e-6 eager, 5e-4 replayed).
    Flag on: one tick per optimiser step, the scheduled form called with exactly the job lists the unscheduled form got (so
    ceil(jobs / 64) launches each), and no unscheduled call."""
    _three_iterations(*make(schedule=None), strip=True)                            # burn-in
    calls, plain = _counted(lambda: _three_iterations(*make(schedule=None), strip=True))
    assert all(calls[n] == [] for n in NEW), calls
    calls, off = _counted(lambda: _three_iterations(*make(schedule=None)))
    assert all(calls[n] == [] for n in NEW), calls
    assert len(calls['t2v_adam_multi']) == 6 and calls['t2v_sgd_multi'] == []      # 3 Python passes x (D step + G step)
    for i, (a, b) in enumerate(zip(off, plain)):
        print('iteration %d: lr_sched=None %s | no attribute %s' % (i, a, b))
        tol = 5e-6 if i < 2 else 5e-4
        assert abs(a[0] - b[0]) < tol and abs(a[1] - b[1]) < tol, (i, a, b)
    unscheduled = calls['t2v_adam_multi']
    parts = make(schedule=('cosine', 100, 1, 0.1))
    calls, _ = _counted(lambda: _three_iterations(*parts))
    assert calls['t2v_lr_tick'] == [0] * 6                                         # exactly one tick per optimiser step
    assert calls['t2v_adam_multi_sched'] == unscheduled                            # the same job lists: ceil(jobs / 64) launches
    assert sum((n + 63) // 64 for n in calls['t2v_adam_multi_sched']) == sum((n + 63) // 64 for n in unscheduled)
    print('jobs per optimiser step:', unscheduled)
    assert calls['t2v_adam_multi'] == [] and calls['t2v_sgd_multi'] == [] and calls['t2v_sgd_multi_sched'] == []
    assert parts[5].counters() == {'D': 3, 'G': 3}


def test_sgd_takes_the_scheduled_form():
    """--sgd composes: the tick and t2v_sgd_multi_sched. Three eager updates under a decay to 0 in two iterations against a twin
    SGD without a schedule whose rate is set to the float product by hand: bit for bit; the third leaves the tensor alone while
    the momentum buffer moves."""
    from txt2vid_amd.gan.lr_sched import LrSchedule
    from txt2vid_amd.optim import SGD
    g = torch.Generator()
    g.manual_seed(5)
    start = torch.randn(5000, generator=g)
    p, q = torch.nn.Parameter(start.clone().to(DEV)), torch.nn.Parameter(start.clone().to(DEV))
    other = torch.nn.Parameter(torch.zeros(3).to(DEV))
    optA, optB, twin = SGD([p], lr=0.1, momentum=0.5), SGD([other], lr=0.1, momentum=0.5), SGD([q], lr=0.1, momentum=0.5)
    sched = LrSchedule('linear', 2, 0, 0.0, 1, 1, DEV).attach(optA, optB)
    seen, bufs = [], []
    for k in range(3):
        grad = torch.randn(5000, generator=g).to(DEV)
        p.grad, q.grad = grad.clone(), grad.clone()
        calls, _ = _counted(optA.step)
        assert calls['t2v_lr_tick'] == [0] and calls['t2v_sgd_multi_sched'] == [1] and calls['t2v_sgd_multi'] == []
        twin.param_groups[0]['lr'] = float(np.float32(0.1) * np.float32(L.factor('linear', k, 0, 2, 0.0)))
        calls, _ = _counted(twin.step)
        assert calls['t2v_lr_tick'] == [] and calls['t2v_sgd_multi_sched'] == [] and calls['t2v_sgd_multi'] == [1]
        assert torch.equal(p.detach(), q.detach()), k
        assert torch.equal(optA.state[p]['momentum_buffer'], twin.state[q]['momentum_buffer']), k
        seen.append(p.detach().clone())
        bufs.append(optA.state[p]['momentum_buffer'].clone())
    assert not torch.equal(seen[0], start.to(DEV)) and not torch.equal(seen[1], seen[0])
    assert torch.equal(seen[2].view(torch.int32), seen[1].view(torch.int32))          # the rate is 0
    assert not torch.equal(bufs[2], bufs[1])
    assert sched.counters() == {'D': 3, 'G': 0}
    assert optA.param_groups[0]['lr'] == 0.1


# ------------------------------------------------------------------------------------------------ 9. command line
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
    linear = ['--lr_decay', 'linear', '--lr_decay_iters', '8']

    def run(args):
        p = subprocess.run([sys.executable, '-m', 'txt2vid_amd.train.gan'] + base + args, cwd=ROOT, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=600)
        out = p.stdout.decode(errors='replace')
        assert p.returncode == 0, out[-3000:]
        return out

    def rates(log):
        """{loop iteration: (schedule iteration, factor, D rate, G rate)} from the log."""
        pat = r'Iter (\d+), learning rates \(--lr_decay \w+, iteration (\d+) of the schedule, factor (\S+)\): D (\S+) G (\S+)'
        return {int(m[0]): (int(m[1]), float(m[2]), float(m[3]), float(m[4])) for m in re.findall(pat, log)}

    def close(a, b):
        return abs(a - b) <= 1e-5 * abs(b)
    out1 = str(tmp_path / 'out1')
    log = run(['--out', out1, '--out_samples', str(tmp_path / 's1'), '--max_iters', '4', '--save_model_period', '4'] + linear)
    got = rates(log)
    assert sorted(got) == [1, 2, 3, 4], log[-3000:]
    for i in range(1, 5):
        f = L.factor('linear', i - 1, 0, 8, 0.0)
        assert got[i][0] == i and close(got[i][1], f) and close(got[i][2], 0.0004 * f) and close(got[i][3], 0.0002 * f), got
    ck = glob.glob(os.path.join(out1, 'iter_4_lossG_*'))
    assert len(ck) == 1
    sd = torch.load(ck[0], map_location='cpu', weights_only=False)
    assert sd['lr_sched']['D'] == 4 and sd['lr_sched']['G'] == 4
    assert sd['lr_sched']['config'] == {'kind': 'linear', 'start': 0, 'end': 8, 'final': 0.0, 'spi': {'D': 1, 'G': 1}}
    assert sd['optD']['param_groups'][0]['lr'] == 0.0004 and sd['optG']['param_groups'][0]['lr'] == 0.0002      # the base rates
    # resume for four more iterations: the first of them is iteration 5 of the schedule, at half the base rates
    out2 = str(tmp_path / 'out2')
    log = run(['--out', out2, '--out_samples', str(tmp_path / 's2'), '--weights', ck[0], '--max_iters', '4', '--save_model_period', '4']
              + linear)
    assert 'D at update 4, G at update 4' in log and 'no lr_sched key' not in log and 'flags win' not in log
    got = rates(log)
    assert got[1][0] == 5 and got[1][1] == 0.5 and close(got[1][2], 0.0002) and close(got[1][3], 0.0001), got
    assert got[4][0] == 8 and close(got[4][1], 0.125)
    ck2 = glob.glob(os.path.join(out2, 'iter_4_lossG_*'))
    assert len(ck2) == 1
    sd2 = torch.load(ck2[0], map_location='cpu', weights_only=False)
    assert sd2['lr_sched']['D'] == 8 and sd2['lr_sched']['G'] == 8
    # the same file without the key: the schedule starts from the file's iteration and says so
    bare = str(tmp_path / 'bare.pt')
    torch.save({k: v for k, v in sd.items() if k != 'lr_sched'}, bare)
    log = run(['--out', str(tmp_path / 'out3'), '--out_samples', str(tmp_path / 's3'), '--weights', bare, '--max_iters', '1',
               '--save_model_period', '0'] + linear)
    assert 'no lr_sched key' in log and 'D at update 4, G at update 4' in log
    assert rates(log)[1][:2] == (5, 0.5)
    # other flags than the file's: reported, and the flags win
    log = run(['--out', str(tmp_path / 'out4'), '--out_samples', str(tmp_path / 's4'), '--weights', ck[0], '--max_iters', '1',
               '--save_model_period', '0', '--lr_decay', 'cosine', '--lr_decay_iters', '16'])
    assert 'flags win' in log and 'D at update 4, G at update 4' in log
    got = rates(log)
    assert got[1][0] == 5 and close(got[1][1], L.factor('cosine', 4, 0, 16, 0.0))
