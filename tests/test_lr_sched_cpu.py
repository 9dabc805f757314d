"""CPU: the learning-rate schedule (--lr_decay) —
  (1) the formula of tests/lr_cases.py is what a `torch.optim.lr_scheduler.LambdaLR` stepped once per iteration applies, for a
      1:1 and a 2:1 step schedule, and the package's host mirror is the same formula;
  (2) the flags and every refusal;
  (3) the C ABI refuses invalid arguments before any launch (no GPU needed);
  (4) the host-only parts of the scheduler object: checkpoint round trip, a file without the key, mismatching flags."""
import ctypes as C
import math

import pytest
import torch

import lr_cases as L

BASE = 2e-3


# ------------------------------------------------------------------------------------------------ 1. the formula
@pytest.mark.parametrize('kind', L.KINDS)
def test_ends_are_exact_and_the_middle_is_the_formula(kind):
    for it in range(0, L.S + 1):
        assert L.factor(kind, it) == 1.0
    for it in range(L.T, L.T + 4):
        assert L.factor(kind, it) == L.F
    for it in range(L.S + 1, L.T):
        frac = (it - L.S) / (L.T - L.S)
        want = 1 - (1 - L.F) * frac if kind == 'linear' else L.F + (1 - L.F) * 0.5 * (1 + math.cos(math.pi * frac))
        assert L.F < L.factor(kind, it) < 1.0
        assert abs(L.factor(kind, it) - want) <= 2 ** -52
    # T = 100000, S = 0, F = 0 (the TGANv2 recipe): half-way is a half
    assert L.factor('linear', 50000, 0, 100000, 0.0) == 0.5
    assert abs(L.factor('cosine', 50000, 0, 100000, 0.0) - 0.5) <= 2 ** -52


@pytest.mark.parametrize('kind', L.KINDS)
def test_host_mirror_is_the_same_formula(kind):
    from txt2vid_amd.gan import lr_sched
    for start, end, final in ((L.S, L.T, L.F), (0, 8, 0.0), (3, 100, 1.0), (0, 1, 0.25)):
        s = lr_sched.LrSchedule(kind, end, start, final)
        for it in range(0, end + 5):
            got, want = s.factor(it), L.factor(kind, it, start, end, final)
            assert abs(got - want) <= 2 ** -52, (it, got, want)
            if it <= start:
                assert got == 1.0
            if it >= end:
                assert got == final


def _toy(spi, make_hooks):
    """Two tensors, `spi` Adam updates per iteration, eight iterations, float64 on the CPU. `make_hooks(opt)` returns
    (before_update(k), after_iteration()); returns the final tensors and the rate each update ran with."""
    g = torch.Generator()
    g.manual_seed(7)
    w = torch.randn(3, 2, generator=g, dtype=torch.float64).requires_grad_()
    b = torch.randn(2, generator=g, dtype=torch.float64).requires_grad_()
    x = torch.randn(16, 3, generator=g, dtype=torch.float64)
    y = torch.randn(16, 2, generator=g, dtype=torch.float64)
    opt = torch.optim.Adam([w, b], lr=BASE, betas=(0.5, 0.999))
    before_update, after_iteration = make_hooks(opt)
    rates, k = [], 0
    for it in range(8):
        for _ in range(spi):
            before_update(k)
            rates.append(opt.param_groups[0]['lr'])
            opt.zero_grad()
            ((x @ w + b - y) ** 2).mean().backward()
            opt.step()
            k += 1
        after_iteration()
    return w.detach(), b.detach(), rates


@pytest.mark.parametrize('spi', [1, 2])
@pytest.mark.parametrize('kind', L.KINDS)
def test_formula_is_a_host_scheduler_stepped_once_per_iteration(kind, spi):
    """`torch.optim.Adam` + `LambdaLR(factor)` stepped once per ITERATION against the same Adam given base * factor(k // spi)
    before its update k: the same rates, update for update, and the same tensors."""
    def scheduled(opt):
        sch = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: L.factor(kind, it))

        def before_update(k):
            assert sch.get_last_lr()[0] == opt.param_groups[0]['lr']
        return before_update, sch.step

    def by_update(opt):
        def before_update(k):
            opt.param_groups[0]['lr'] = BASE * L.update_factors(kind, spi, k + 1)[k]
        return before_update, lambda: None
    w1, b1, r1 = _toy(spi, scheduled)
    w2, b2, r2 = _toy(spi, by_update)
    assert r1 == r2
    assert torch.equal(w1, w2) and torch.equal(b1, b2)
    fs = L.update_factors(kind, spi, 8 * spi)
    assert len(r1) == 8 * spi
    for k, (r, f) in enumerate(zip(r1, fs)):
        assert r == BASE * f and abs(r / BASE - f) <= 2 ** -52, (k, r, f)
        assert f == L.factor(kind, k // spi)
    # the updates of one iteration share one factor; the ends are exactly 1 and F
    for it in range(8):
        assert len(set(fs[it * spi:(it + 1) * spi])) == 1
    assert fs[:(L.S + 1) * spi] == [1.0] * ((L.S + 1) * spi)
    assert fs[L.T * spi:] == [L.F] * ((8 - L.T) * spi)


# ------------------------------------------------------------------------------------------------ 2. flags
NEEDED = ['--data', 'd.json', '--G', 'g', '--D', 'd']


def _args(extra):
    from txt2vid_amd.train.gan import build_parser
    return build_parser().parse_args(NEEDED + extra)


def test_defaults_are_off():
    from txt2vid_amd.gan import lr_sched
    a = _args([])
    assert a.lr_decay == 'none'
    assert lr_sched.check_args(a) is a
    assert (a.lr_decay_iters, a.lr_decay_start, a.lr_final) == (None, None, None)

    class Bare(object):                                  # parameter objects without the attributes mean "off"
        pass
    lr_sched.check_args(Bare())


def test_accepted_flags_resolve_their_defaults():
    from txt2vid_amd.gan import lr_sched
    a = lr_sched.check_args(_args(['--lr_decay', 'linear', '--lr_decay_iters', '100000']))
    assert (a.lr_decay, a.lr_decay_iters, a.lr_decay_start, a.lr_final) == ('linear', 100000, 0, 0.0)
    a = lr_sched.check_args(_args(['--lr_decay', 'cosine', '--lr_decay_iters', '5', '--lr_decay_start', '2', '--lr_final', '0.1']))
    assert (a.lr_decay, a.lr_decay_iters, a.lr_decay_start, a.lr_final) == ('cosine', 5, 2, 0.1)
    for f in ('0', '1'):
        lr_sched.check_args(_args(['--lr_decay', 'linear', '--lr_decay_iters', '5', '--lr_final', f]))


@pytest.mark.parametrize('extra', [
    ['--lr_decay', 'linear'],                                                              # a decay without its end
    ['--lr_decay', 'cosine'],
    ['--lr_decay', 'linear', '--lr_decay_iters', '5', '--lr_decay_start', '5'],            # T <= S
    ['--lr_decay', 'linear', '--lr_decay_iters', '4', '--lr_decay_start', '5'],
    ['--lr_decay', 'linear', '--lr_decay_iters', '0'],
    ['--lr_decay', 'linear', '--lr_decay_iters', '5', '--lr_decay_start', '-1'],           # S < 0
    ['--lr_decay', 'linear', '--lr_decay_iters', '5', '--lr_final', '-0.01'],              # F outside [0, 1]
    ['--lr_decay', 'cosine', '--lr_decay_iters', '5', '--lr_final', '1.01'],
    ['--lr_decay', 'linear', '--lr_decay_iters', '5', '--lr_final', 'nan'],
    ['--lr_decay_iters', '5'],                                                             # numeric flags without a decay
    ['--lr_decay_start', '0'],
    ['--lr_final', '0'],
    ['--lr_decay', 'none', '--lr_decay_iters', '5'],
    ['--lr_decay', 'linear', '--lr_decay_iters', str(2 ** 23), '--discrim_steps', '2'],    # past the exact range of the count
])
def test_refusals(extra):
    from txt2vid_amd.gan import lr_sched
    with pytest.raises(ValueError):
        lr_sched.check_args(_args(extra))


def test_unknown_kind_is_refused_by_the_parser():
    with pytest.raises(SystemExit):
        _args(['--lr_decay', 'exponential', '--lr_decay_iters', '5'])


def test_main_refuses_before_anything_is_built(monkeypatch):
    """`train.gan.main` raises on a bad schedule before it touches the process group, the device or the data."""
    from txt2vid_amd.train import gan as cli
    from txt2vid_amd import dist
    monkeypatch.setattr(dist, 'init_from_env', lambda *a, **k: pytest.fail('a process group was formed'))
    with pytest.raises(ValueError, match='lr_decay_iters'):
        cli.main(_args(['--lr_decay', 'linear']))


# ------------------------------------------------------------------------------------------------ 3. C ABI
def test_c_abi_refuses_invalid_arguments_without_a_gpu():
    from txt2vid_amd._lib import lib, AdamJob
    l = lib()
    state = (C.c_float * 2)(0.0, 1.0)                    # host memory: never dereferenced, every call below returns first
    sp = C.cast(state, C.c_void_p)
    assert l.t2v_lr_tick(None, 1, 0, 5, 0.0, 1, None) == -1            # NULL state
    assert l.t2v_lr_tick(sp, 0, 0, 5, 0.0, 1, None) == -1              # unknown kind
    assert l.t2v_lr_tick(sp, 3, 0, 5, 0.0, 1, None) == -1
    assert l.t2v_lr_tick(sp, 1, 5, 5, 0.0, 1, None) == -1              # T <= S
    assert l.t2v_lr_tick(sp, 2, 6, 5, 0.0, 1, None) == -1
    assert l.t2v_lr_tick(sp, 1, -1, 5, 0.0, 1, None) == -1             # S < 0
    assert l.t2v_lr_tick(sp, 1, 0, 5, 0.0, 0, None) == -1              # spi < 1
    assert l.t2v_lr_tick(sp, 1, 0, 5, 1.5, 1, None) == -1              # F outside [0, 1]
    assert l.t2v_lr_tick(sp, 1, 0, 5, float('nan'), 1, None) == -1
    assert list(state) == [0.0, 1.0]
    buf = (C.c_float * 8)()
    bp = C.cast(buf, C.c_void_p).value

    def job(p, g, m, v, n):
        arr = (AdamJob * 1)()
        arr[0].p, arr[0].g, arr[0].m, arr[0].v, arr[0].n = p, g, m, v, n
        return arr
    ok = job(bp, bp, bp, bp, 8)
    adam = lambda jobs, n, scale: l.t2v_adam_multi_sched(jobs, n, 1e-3, scale, 0.5, 0.999, 1e-8, 0.5, 1e-3, 1.0, None, None)
    sgd = lambda jobs, n, scale, mu=0.5: l.t2v_sgd_multi_sched(jobs, n, 1e-3, scale, mu, 1.0, 0, None)
    for f in (adam, sgd):
        assert f(None, 1, sp) == -1                      # NULL jobs
        assert f(ok, 0, sp) == -1                        # no jobs
        assert f(ok, 1, None) == -1                      # NULL schedule state
        assert f(job(None, bp, bp, bp, 8), 1, sp) == -1
        assert f(job(bp, None, bp, bp, 8), 1, sp) == -1
        assert f(job(bp, bp, bp, bp, 0), 1, sp) == -1
        assert f(job(bp, bp, bp, bp, 2 ** 31), 1, sp) == -1
    assert adam(job(bp, bp, None, bp, 8), 1, sp) == -1
    assert adam(job(bp, bp, bp, None, 8), 1, sp) == -1
    assert sgd(job(bp, bp, None, None, 8), 1, sp) == -1  # momentum without a buffer
    assert list(buf) == [0.0] * 8


# ------------------------------------------------------------------------------------------------ 4. the scheduler object, host side
def test_attach_and_constructor_refusals():
    from txt2vid_amd.gan.lr_sched import LrSchedule
    from txt2vid_amd.optim import Adam, SGD
    for Opt in (Adam, SGD):
        a, b = Opt([torch.zeros(2, requires_grad=True)], lr=1e-3), Opt([torch.zeros(2, requires_grad=True)], lr=2e-3)
        assert a.lr_sched is None and b.lr_sched is None
        s = LrSchedule('linear', 5, 2, 0.1, n_d=2, n_g=1).attach(a, b)
        assert a.lr_sched.state is s.state['D'] and b.lr_sched.state is s.state['G']
        assert (a.lr_sched.spi, b.lr_sched.spi) == (2, 1)
        assert a.param_groups[0]['lr'] == 1e-3 and b.param_groups[0]['lr'] == 2e-3      # the base rates stay visible
        with pytest.raises(RuntimeError):
            a.lr_sched.tick()                            # no CPU fallback
    for bad in (('step', 5), ('linear', 5, 5), ('linear', 5, -1), ('linear', 5, 0, 1.5), ('linear', 5, 0, 0.0, 0, 1),
                ('linear', 2 ** 24, 0, 0.0)):
        with pytest.raises(ValueError):
            LrSchedule(*bad)


def test_checkpoint_round_trip_on_the_host():
    from txt2vid_amd.gan.lr_sched import LrSchedule
    s = LrSchedule('linear', 8, n_d=2, n_g=1)
    assert s.state_dict() == {'D': 0, 'G': 0, 'config': {'kind': 'linear', 'start': 0, 'end': 8, 'final': 0.0, 'spi': {'D': 2, 'G': 1}}}
    assert s.load_state_dict({'D': 8, 'G': 4, 'config': s.config()}) == []
    assert s.counters() == {'D': 8, 'G': 4}
    d_ptr = s.state['D'].data_ptr()
    # a file without the key: from the file's iteration, and it says so
    notes = s.load_state_dict(None, iteration=3)
    assert s.counters() == {'D': 6, 'G': 3} and len(notes) == 1 and 'no lr_sched key' in notes[0]
    assert s.load_state_dict(None, iteration=0) == [] and s.counters() == {'D': 0, 'G': 0}
    # another configuration in the file: reported, the flags win, the counters are taken over
    other = LrSchedule('cosine', 9, n_d=2, n_g=1)
    notes = other.load_state_dict(s.state_dict() | {'D': 10, 'G': 5})
    assert len(notes) == 1 and 'flags win' in notes[0]
    assert other.counters() == {'D': 10, 'G': 5} and other.kind == 'cosine' and other.end == 9
    assert s.state['D'].data_ptr() == d_ptr              # loaded in place
    with pytest.raises(ValueError):
        s.load_state_dict({'D': -1, 'G': 0})


def test_train_step_refuses_a_schedule_counting_other_steps():
    from txt2vid_amd.gan.lr_sched import LrSchedule
    from txt2vid_amd.gan.trainer import TrainStep
    from txt2vid_amd.optim import Adam
    optD, optG = Adam([torch.zeros(2, requires_grad=True)]), Adam([torch.zeros(2, requires_grad=True)])
    LrSchedule('linear', 8, n_d=1, n_g=1).attach(optD, optG)

    class Prm(object):
        discrim_steps, gen_steps = 2, 1

    class Gan(object):
        gen = None
    with pytest.raises(ValueError, match='--discrim_steps'):
        TrainStep(Gan(), optD, optG, None, Prm(), 'cpu')
