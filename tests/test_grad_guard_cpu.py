"""Host side of the gradient guard (--grad_guard / --D_clip / --G_clip) —
  (1) the flag rules: every refusal, the implied --grad_guard, the parser round trip;
  (2) the host mirror of the coefficient against torch.nn.utils.clip_grad_norm_ in float64;
  (3) state_dict / load_state_dict: round trip, a missing key, a negative count;
  (4) the C ABI refuses invalid arguments before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import guard_cases as G

NEEDED = ['--data', 'd.json', '--G', 'g', '--D', 'd']


def _args(extra):
    from txt2vid_amd.train.gan import build_parser
    return build_parser().parse_args(NEEDED + extra)


# ------------------------------------------------------------------------------------------------ 1. flags
def test_defaults_are_off():
    from txt2vid_amd.gan import grad_guard
    a = _args([])
    assert (a.grad_guard, a.D_clip, a.G_clip) == (False, None, None)
    assert grad_guard.check_args(a) is a and not grad_guard.enabled(a)
    assert (a.grad_guard, a.D_clip, a.G_clip) == (False, None, None)

    class Bare(object):                                  # parameter objects without the attributes mean "off"
        pass
    grad_guard.check_args(Bare())
    assert not grad_guard.enabled(Bare())


@pytest.mark.parametrize('extra, want', [
    (['--grad_guard'], (True, None, None)),
    (['--D_clip', '2.5'], (True, 2.5, None)),                                  # either clip flag implies --grad_guard
    (['--G_clip', '1e30'], (True, None, 1e30)),
    (['--D_clip', '1', '--G_clip', '0.5', '--grad_guard'], (True, 1.0, 0.5)),
    (['--G_clip', '1', '--sgd', '--D_sn', '--lr_decay', 'linear', '--lr_decay_iters', '9', '--no_graph', '--gen_steps', '2'],
     (True, None, 1.0)),
])
def test_parser_round_trip(extra, want):
    from txt2vid_amd.gan import grad_guard
    a = grad_guard.check_args(_args(extra))
    assert (a.grad_guard, a.D_clip, a.G_clip) == want and grad_guard.enabled(a)


@pytest.mark.parametrize('extra', [
    ['--D_clip', '0'], ['--D_clip', '-1'], ['--D_clip', 'inf'], ['--D_clip', 'nan'],
    ['--G_clip', '0'], ['--G_clip', '-0.5'], ['--G_clip', 'inf'], ['--G_clip', 'nan'],
    ['--grad_guard', '--max_iters', str(2 ** 23), '--discrim_steps', '2'],          # past the exact range of the float counts
])
def test_refusals(extra):
    from txt2vid_amd.gan import grad_guard
    with pytest.raises(ValueError):
        grad_guard.check_args(_args(extra))


@pytest.mark.parametrize('extra', [['--grad_guard'], ['--D_clip', '1'], ['--G_clip', '1']])
def test_end2end_is_refused(extra):
    from txt2vid_amd.gan import grad_guard
    with pytest.raises(NotImplementedError, match='end2end'):
        grad_guard.check_args(_args(extra + ['--end2end']))
    grad_guard.check_args(_args(['--end2end']))          # without the flags nothing is refused


def test_main_refuses_before_anything_is_built(monkeypatch):
    from txt2vid_amd.train import gan as cli
    from txt2vid_amd import dist
    monkeypatch.setattr(dist, 'init_from_env', lambda *a, **k: pytest.fail('a process group was formed'))
    with pytest.raises(ValueError, match='D_clip'):
        cli.main(_args(['--D_clip', '0']))


# ------------------------------------------------------------------------------------------------ 2. host mirror
@pytest.mark.parametrize('norm, clip', [(0.5, 1.0), (1.0 - 1e-3, 1.0), (1.0, 1.0), (1.0 + 1e-3, 1.0), (37.5, 1.0), (1e6, 0.01),
                                        (3.0, 3.0), (1e-3, 5.0)])
def test_host_mirror_is_clip_grad_norm(norm, clip):
    """float32 formula against torch's float64 one: one division and one addition in float32, so 3 float32 roundings
    (norm, sum, quotient): relative 2e-7 is 3 x 2^-24 rounded up. Below the bound the coefficient is exactly 1."""
    from txt2vid_amd.gan import grad_guard
    c, skip = grad_guard.coef(norm, clip)
    want = G.torch_coef64(norm, clip)
    print('norm %g clip %g: mirror %.9g torch float64 %.17g' % (norm, clip, c, want))
    assert not skip and isinstance(c, np.float32)
    assert abs(float(c) - want) <= 2e-7 * want
    assert c == G.coef32(norm, clip)
    if norm + 1e-6 < clip * (1 - 1e-6):
        assert c == np.float32(1.0) and want == 1.0
    if norm > clip * (1 + 1e-6):
        assert c < np.float32(1.0)


def test_host_mirror_skips_non_finite_norms_and_measures_without_a_bound():
    from txt2vid_amd.gan import grad_guard
    for bad in (float('inf'), float('nan')):
        assert grad_guard.coef(bad, 1.0) == (np.float32(1.0), True)
        assert grad_guard.coef(bad, None) == (np.float32(1.0), True)
    assert grad_guard.coef(1e9, None) == (np.float32(1.0), False)
    assert grad_guard.coef(1e9, 0.0) == (np.float32(1.0), False)


# ------------------------------------------------------------------------------------------------ 3. the object, host side
def test_attach_and_constructor_refusals():
    from txt2vid_amd.gan.grad_guard import GradGuard
    from txt2vid_amd.optim import Adam, SGD
    for Opt in (Adam, SGD):
        a, b = Opt([torch.zeros(5000, requires_grad=True)], lr=1e-3), Opt([torch.zeros(2, 3, 3, 3, requires_grad=True)], lr=2e-3)
        assert a.grad_guard is None and b.grad_guard is None
        g = GradGuard(2.0, None).attach(a, b)
        assert a.grad_guard.state is g.state['D'] and b.grad_guard.state is g.state['G']
        assert (a.grad_guard.clip, b.grad_guard.clip) == (2.0, None)
        assert g.state['D'].tolist() == [1.0] + [0.0] * 7 and g.state['D'].dtype == torch.float32
        assert a.grad_guard.partials.numel() >= 2 and b.grad_guard.partials.numel() >= 9
        with pytest.raises(RuntimeError):
            a.grad_guard.measure(None, 0, 1.0)           # no CPU fallback
    for bad in ((0.0, None), (None, -1.0), (float('inf'), None), (None, float('nan'))):
        with pytest.raises(ValueError):
            GradGuard(*bad)


def test_checkpoint_round_trip_on_the_host():
    from txt2vid_amd.gan.grad_guard import GradGuard
    g = GradGuard(2.0, None)
    zero = {'steps': 0, 'skipped': 0, 'clipped': 0}
    assert g.state_dict() == {'D': zero, 'G': zero, 'config': {'clip_D': 2.0, 'clip_G': None}}
    d_ptr = g.state['D'].data_ptr()
    sd = {'D': {'steps': 8, 'skipped': 1, 'clipped': 5}, 'G': {'steps': 4, 'skipped': 0, 'clipped': 0}, 'config': g.config()}
    assert g.load_state_dict(sd) == []
    assert g.state_dict() == sd and g.counters() == {'D': sd['D'], 'G': sd['G']}
    assert g.state['D'].tolist() == [1.0, 0.0, 0.0, 8.0, 1.0, 5.0, 0.0, 0.0]
    # a file without the key: from zero, and it says so
    notes = g.load_state_dict(None)
    assert g.counters() == {'D': zero, 'G': zero} and len(notes) == 1 and 'no grad_guard key' in notes[0]
    # other bounds in the file: reported, the flags win, the counts are taken over
    other = GradGuard(None, 1.0)
    notes = other.load_state_dict(sd)
    assert len(notes) == 1 and 'flags win' in notes[0]
    assert other.counters() == {'D': sd['D'], 'G': sd['G']} and other.config() == {'clip_D': None, 'clip_G': 1.0}
    assert g.state['D'].data_ptr() == d_ptr              # loaded in place
    with pytest.raises(ValueError):
        g.load_state_dict({'D': {'steps': 3, 'skipped': -1, 'clipped': 0}, 'G': zero})
    with pytest.raises(ValueError):
        g.load_state_dict({'D': {'steps': 2 ** 24, 'skipped': 0, 'clipped': 0}, 'G': zero})


def test_log_line_parses():
    from txt2vid_amd.gan.grad_guard import log_line, unpack
    line = log_line(7, unpack([0.5, 0.0, 3.25, 7.0, 1.0, 2.0]), unpack([1.0, 1.0, float('nan'), 7.0, 3.0, 0.0]))
    assert line == 'Iter 7, gradient guard: norm D 3.25 G nan, coef D 0.5 G 1, skipped D 1 G 3, clipped D 2 G 0'


# ------------------------------------------------------------------------------------------------ 4. C ABI
def test_c_abi_refuses_invalid_arguments_without_a_gpu():
    from txt2vid_amd._lib import lib, AdamJob
    l = lib()
    state = (C.c_float * 8)(1.0)                         # host memory: never dereferenced, every call below returns first
    sp = C.cast(state, C.c_void_p)
    buf = (C.c_float * 8)()
    bp = C.cast(buf, C.c_void_p).value

    def job(p, g, m, v, n):
        arr = (AdamJob * 1)()
        arr[0].p, arr[0].g, arr[0].m, arr[0].v, arr[0].n = p, g, m, v, n
        return arr
    ok = job(bp, bp, bp, bp, 8)
    assert l.t2v_grad_sumsq_multi(None, 1, 1.0, sp, None) == -1               # NULL jobs
    assert l.t2v_grad_sumsq_multi(ok, 0, 1.0, sp, None) == -1                 # no jobs
    assert l.t2v_grad_sumsq_multi(ok, 1, 1.0, None, None) == -1               # NULL partials
    assert l.t2v_grad_sumsq_multi(job(None, None, None, None, 8), 1, 1.0, sp, None) == -1     # NULL gradient
    assert l.t2v_grad_sumsq_multi(job(None, bp, None, None, 0), 1, 1.0, sp, None) == -1       # n < 1
    assert l.t2v_grad_sumsq_multi(job(None, bp, None, None, 2 ** 31), 1, 1.0, sp, None) == -1
    assert l.t2v_grad_guard(None, 1, 1.0, sp, None) == -1
    assert l.t2v_grad_guard(sp, 0, 1.0, sp, None) == -1                       # no chunks
    assert l.t2v_grad_guard(sp, 1, 1.0, None, None) == -1
    assert l.t2v_grad_guard(sp, 1, float('nan'), sp, None) == -1
    assert l.t2v_adam_tick_guard(None, 0.5, 0.999, sp, None) == -1
    assert l.t2v_adam_tick_guard(sp, 0.5, 0.999, None, None) == -1
    adam = lambda jobs, n, gd, sc=None: l.t2v_adam_multi_guard(jobs, n, 1e-3, sc, 0.5, 0.999, 1e-8, 0.5, 1e-3, 1.0, None, gd, None)
    sgd = lambda jobs, n, gd, sc=None, mu=0.5: l.t2v_sgd_multi_guard(jobs, n, 1e-3, sc, mu, 1.0, 0, gd, None)
    for f in (adam, sgd):
        for sc in (None, sp):                            # with and without the schedule pointer
            assert f(None, 1, sp, sc) == -1              # NULL jobs
            assert f(ok, 0, sp, sc) == -1                # no jobs
            assert f(ok, 1, None, sc) == -1              # NULL guard state
            assert f(job(None, bp, bp, bp, 8), 1, sp, sc) == -1
            assert f(job(bp, None, bp, bp, 8), 1, sp, sc) == -1
            assert f(job(bp, bp, bp, bp, 0), 1, sp, sc) == -1
            assert f(job(bp, bp, bp, bp, 2 ** 31), 1, sp, sc) == -1
    assert adam(job(bp, bp, None, bp, 8), 1, sp) == -1
    assert adam(job(bp, bp, bp, None, 8), 1, sp) == -1
    assert sgd(job(bp, bp, None, None, 8), 1, sp) == -1  # momentum without a buffer
    assert list(buf) == [0.0] * 8 and list(state) == [1.0] + [0.0] * 7
