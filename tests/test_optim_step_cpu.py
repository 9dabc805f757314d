"""CPU: the order of the launches of one optimiser step, for every combination of {no extra, --lr_decay, --grad_guard, both} x
{with, without a --D_sn weight hook} x {Adam, SGD}. The entry points of the library and the host-side helpers around them are
replaced by recorders; the expected sequences below are written out from the step as it stood before Adam and SGD shared its
skeleton (they pass there too), so they pin the interleaving whoever owns it:
  flush, projection | tick first without a guard; with one: measure everything, then tick | update | refresh, re-pack."""
import pytest
import torch

from txt2vid_amd import functional as TF
from txt2vid_amd.gan.grad_guard import GradGuard
from txt2vid_amd.gan.lr_sched import LrSchedule
from txt2vid_amd.optim import Adam, SGD

WITH_JOBS = ('t2v_adam_multi', 't2v_adam_multi_sched', 't2v_adam_multi_guard', 't2v_sgd_multi', 't2v_sgd_multi_sched',
             't2v_sgd_multi_guard', 't2v_grad_sumsq_multi')
MEASURE = ['t2v_grad_sumsq_multi:2', 't2v_grad_guard']
TAIL = ['bump_weight_epoch', 'repack_params']

# the launches between the preamble (flush, projection) and the postamble (refresh, bump, re-pack), state already allocated
BODY = {
    (Adam, 'none'): ['t2v_adam_tick', 't2v_adam_multi:2'],
    (Adam, 'sched'): ['t2v_adam_tick', 't2v_lr_tick', 't2v_adam_multi_sched:2'],
    (Adam, 'guard'): MEASURE + ['t2v_adam_tick_guard', 't2v_adam_multi_guard:2'],
    (Adam, 'sched+guard'): MEASURE + ['t2v_adam_tick_guard', 't2v_lr_tick', 't2v_adam_multi_guard:2'],
    (SGD, 'none'): ['t2v_sgd_multi:2'],
    (SGD, 'sched'): ['t2v_lr_tick', 't2v_sgd_multi_sched:2'],
    (SGD, 'guard'): MEASURE + ['t2v_sgd_multi_guard:2'],
    (SGD, 'sched+guard'): MEASURE + ['t2v_lr_tick', 't2v_sgd_multi_guard:2'],
}
# the first step allocates the state: Adam two moments per parameter (fill launches) behind its tick, in front of the guard's
# measurement; SGD's momentum buffers are filled only under a guard (the first step may be the skipped one)
FIRST = {
    (Adam, 'none'): ['t2v_adam_tick'] + ['zeros_like'] * 4 + ['t2v_adam_multi:2'],
    (Adam, 'sched+guard'): ['zeros_like'] * 4 + MEASURE + ['t2v_adam_tick_guard', 't2v_lr_tick', 't2v_adam_multi_guard:2'],
    (SGD, 'none'): ['t2v_sgd_multi:2'],
    (SGD, 'sched+guard'): ['zeros_like'] * 2 + MEASURE + ['t2v_lr_tick', 't2v_sgd_multi_guard:2'],
}
# no gradient anywhere: nothing to measure, the guard is dropped and the tick is the plain one
IDLE = {
    (Adam, 'guard'): ['t2v_adam_tick'],
    (Adam, 'sched+guard'): ['t2v_adam_tick', 't2v_lr_tick'],
    (SGD, 'guard'): [],
    (SGD, 'sched+guard'): ['t2v_lr_tick'],
}


class _Dev(object):
    """Stands in for a device tensor: the host code asks where it lives, how long it is and for its address."""
    is_cuda = True

    def __init__(self, t):
        self.t = t

    def data_ptr(self):
        return self.t.data_ptr()

    def numel(self):
        return self.t.numel()


class _Hook(object):
    def __init__(self, log):
        self.log = log

    def project_grads(self):
        self.log.append('project_grads')

    def refresh(self, touched):
        self.log.append('refresh')
        return touched


@pytest.fixture
def log(monkeypatch):
    log = []

    class Lib(object):
        def __getattr__(self, name):
            def entry(*a):
                log.append(name + (':%d' % a[1] if name in WITH_JOBS else ''))
                return 0
            return entry
    fake = Lib()
    monkeypatch.setattr(TF, 'lib', lambda: fake)
    monkeypatch.setattr(TF, '_stream', lambda: None)
    monkeypatch.setattr(TF, 'grad_sink_flush', lambda: log.append('grad_sink_flush'))
    monkeypatch.setattr(TF, 'zeros_like', lambda t: log.append('zeros_like') or torch.zeros_like(t))
    monkeypatch.setattr(TF, 'bump_weight_epoch', lambda ps=None: log.append('bump_weight_epoch'))
    monkeypatch.setattr(TF, 'repack_params', lambda ps: log.append('repack_params'))
    return log


def _make(cls, extras, hook, log):
    """The optimiser over two parameters of 4 and 6 elements, with the device-resident step counter where it has one."""
    ps = [torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(2, 3))]
    kw = {'betas': (0.5, 0.9)} if cls is Adam else {'momentum': 0.5}
    opt, other = cls(ps, lr=1e-3, **kw), cls([torch.nn.Parameter(torch.zeros(1))], lr=1e-3, **kw)
    if cls is Adam:
        opt.step_dev = torch.zeros(3)
    if 'sched' in extras:
        LrSchedule('linear', 100).attach(opt, other)
        opt.lr_sched.state = _Dev(opt.lr_sched.state)
    if 'guard' in extras:
        GradGuard(1.0, None).attach(opt, other)
        opt.grad_guard.state = _Dev(opt.grad_guard.state)
    if hook:
        opt.weight_hook = _Hook(log)
    return opt, ps


def _step(opt, ps, log, grads=True):
    for p in ps:
        p.grad = torch.ones_like(p) if grads else None
    del log[:]
    opt.step()
    return list(log)


@pytest.mark.parametrize('hook', [False, True])
@pytest.mark.parametrize('extras', ['none', 'sched', 'guard', 'sched+guard'])
@pytest.mark.parametrize('cls', [Adam, SGD])
def test_launch_sequence_of_a_step(log, cls, extras, hook):
    opt, ps = _make(cls, extras, hook, log)
    head = ['grad_sink_flush'] + (['project_grads'] if hook else [])
    tail = (['refresh'] if hook else []) + TAIL
    first = _step(opt, ps, log)
    if (cls, extras) in FIRST:
        assert first == head + FIRST[cls, extras] + tail
    assert [n for n in first if n != 'zeros_like'] == head + BODY[cls, extras] + tail
    assert _step(opt, ps, log) == head + BODY[cls, extras] + tail
    if (cls, extras) in IDLE:
        assert _step(opt, ps, log, grads=False) == head + IDLE[cls, extras] + tail
        assert opt.grad_guard is not None                                  # (dropped for that step only)
        assert _step(opt, ps, log) == head + BODY[cls, extras] + tail
