"""CPU: the seam between the training loop and its opt-in features (gan/extras.py) — the ring that reads the losses and the
extras' floats one iteration late, the fixed order of a run's extras, and the log lines the per-feature tests parse. (The KL of
the conditioning augmentation is a loss slot that train() logs itself; the averaged generator and spectral normalisation neither
log nor travel.)"""
import itertools
import re

import pytest
import torch

from txt2vid_amd.gan.ada import AdaState
from txt2vid_amd.gan.extras import Readout, training_extras
from txt2vid_amd.gan.grad_guard import GradGuard
from txt2vid_amd.gan.lr_sched import LrSchedule
from txt2vid_amd.optim import Adam


def _extras(which):
    made = {'ada': AdaState(0.6, p0=0.25), 'lr': LrSchedule('linear', 10), 'guard': GradGuard(2.0, None)}
    return [made[k] for k in which]


@pytest.mark.parametrize('which, width, offsets', [
    ((), 4, {}),
    (('ada',), 4, {'ada.p': 3}),
    (('lr', 'guard'), 16, {'guard.D': 3, 'guard.G': 9}),
    (('ada', 'lr', 'guard'), 16, {'ada.p': 3, 'guard.D': 4, 'guard.G': 10}),
])
def test_offsets_and_width_follow_from_the_slot_list(which, width, offsets):
    """The three loss slots, then every extra's tensors back to back (the schedule has none); the width is the sum rounded up to
    whole 16-byte rows: 4 floats with no extra, as the loop has always had."""
    r = Readout(_extras(which), 'cpu')
    assert [(name, off) for name, off, n, t in r.slots] == [('lD', 0), ('lG', 1), ('kl', 2)] + sorted(offsets.items(), key=lambda s: s[1])
    assert [n for name, off, n, t in r.slots] == [1, 1, 1] + [1 if name == 'ada.p' else 6 for name in sorted(offsets, key=offsets.get)]
    name, off, n, t = r.slots[-1]
    assert r.width == width and off + n <= width < off + n + 4
    assert all(hbuf.numel() == width and not hbuf.is_pinned() and ev is None for hbuf, ev in r.ring)


def test_pop_lags_one_push_and_returns_by_name():
    ada, lr, guard = extras = _extras(('ada', 'lr', 'guard'))
    r = Readout(extras, 'cpu')
    rows = {w: [0.5, 0.0, 3.0 + i, 7.0, 1.0, 2.0, -1.0, -1.0] for i, w in enumerate('DG')}     # (the last two are not read)

    def push(k, kl=True):
        ada.ada[0] = 0.125 * k
        for w in 'DG':
            guard.state[w].copy_(torch.tensor(rows[w]) * k)
        r.push(k, lD=torch.tensor(1.0 * k), lG=torch.tensor(2.0 * k), kl=torch.tensor(3.0 * k) if kl else None)

    def want(k, kl=True):
        return {'lD': [1.0 * k], 'lG': [2.0 * k], 'kl': [3.0 * k if kl else 0.0], 'ada.p': [0.125 * k],
                'guard.D': [v * k for v in rows['D'][:6]], 'guard.G': [v * k for v in rows['G'][:6]]}
    push(1, kl=False)
    assert r.pop() is None                                 # nothing on the first call
    push(2, kl=False)
    assert r.pop() == want(1, kl=False)                    # a loss that is not in the run stays 0
    assert r.pop() == want(1, kl=False)                    # (reading does not consume)
    push(3)
    assert r.pop() == want(2, kl=False)
    push(4)
    assert r.pop() == want(3)
    # by name, not by position: the same values whatever else travels and wherever the slot lies
    alone = Readout([guard], 'cpu')
    alone.push(1, lD=torch.tensor(9.0), lG=torch.tensor(8.0))
    alone.push(2, lD=torch.tensor(9.0), lG=torch.tensor(8.0))
    assert alone.pop() == {'lD': [9.0], 'lG': [8.0], 'kl': [0.0], 'guard.D': want(4)['guard.D'], 'guard.G': want(4)['guard.G']}
    # what the eager loop reads on the spot at its log period: the same tensors under the same names
    assert {name: t[:n].tolist() for e in extras for name, t, n in e.slots} == \
        {k: v for k, v in want(4).items() if k in ('ada.p', 'guard.D', 'guard.G')}
    assert lr.slots == () and (ada.key, lr.key, guard.key) == (None, 'lr_sched', 'grad_guard')


class _Stub(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.mark.parametrize('which', [c for n in range(4) for c in itertools.combinations(('ada', 'lr', 'guard'), n)])
def test_extras_of_a_run_come_in_the_order_of_their_log_lines(which):
    ada, guard = object(), object()
    lr = _Stub(counters=lambda: {'D': 8, 'G': 4}, spi={'D': 2, 'G': 1}, it0=0)
    gan = _Stub(ada=ada if 'ada' in which else None)
    optD, optG = (_Stub(lr_sched=_Stub(sched=lr) if 'lr' in which else None,
                        grad_guard=_Stub(guard=guard) if 'guard' in which else None) for _ in range(2))
    got = training_extras(gan, optD, optG)
    assert [id(e) for e in got] == [id(e) for k, e in (('ada', ada), ('lr', lr), ('guard', guard)) if k in which]
    assert lr.it0 == (4 if 'lr' in which else 0)           # the schedule's log counts on from where its state stands


def test_log_lines_are_the_ones_the_feature_tests_parse():
    """The regular expressions of test_ada_gpu, test_lr_sched_gpu and test_grad_guard_gpu, on lines built here."""
    ada, lr, guard = _extras(('ada', 'lr', 'guard'))
    seen = {}
    assert ada.log_lines(2, seen) == [] and guard.log_lines(2, seen) == []           # nothing read yet: nothing to say
    seen.update({'ada.p': [0.03125], 'guard.D': [0.5, 0.0, 3.25, 7.0, 1.0, 2.0], 'guard.G': [1.0, 1.0, float('nan'), 7.0, 3.0, 0.0]})
    line, = ada.log_lines(2, seen)
    assert line == 'Iter 2, augmentation probability p (--D_ada, target 0.6): 0.0312'
    assert re.search(r'Iter 2, augmentation probability p \(--D_ada, target 0.6\): ([0-9.]+)', line).group(1) == '0.0312'
    assert ada.log_lines(3, {'ada.p': [0.0]}) == ['Iter 3, augmentation probability p (--D_ada, target 0.6): 0.0000']
    line, = guard.log_lines(7, seen)
    assert line == 'Iter 7, gradient guard: norm D 3.25 G nan, coef D 0.5 G 1, skipped D 1 G 3, clipped D 2 G 0'
    pat = (r'Iter (\d+), gradient guard: norm D (\S+) G (\S+), coef D (\S+) G (\S+), skipped D (\d+) G (\d+), '
           r'clipped D (\d+) G (\d+)')
    assert re.findall(pat, line) == [('7', '3.25', 'nan', '0.5', '1', '1', '3', '2', '0')]
    # the schedule: rates from the host mirror, counted on from where the device state stands when train() starts
    lr = LrSchedule('linear', 10, n_d=2, n_g=1)
    optD, optG = (Adam([torch.nn.Parameter(torch.zeros(1))], lr=rate) for rate in (4e-4, 2e-4))
    lr.attach(optD, optG)
    assert training_extras(_Stub(ada=None), optD, optG) == [lr]
    assert lr.log_lines(1, seen) == ['Iter 1, learning rates (--lr_decay linear, iteration 1 of the schedule, factor 1): D 0.0004 G 0.0002']
    lr.load_state_dict({'D': 8, 'G': 4})
    assert lr.log_lines(1, seen)[0].startswith('Iter 1, learning rates (--lr_decay linear, iteration 1 of')      # until a run begins
    assert training_extras(_Stub(ada=None), optD, optG) == [lr]                      # train() starts, 4 iterations in
    line, = lr.log_lines(3, seen)
    assert line == 'Iter 3, learning rates (--lr_decay linear, iteration 7 of the schedule, factor 0.4): D 0.00016 G 8e-05'
    pat = r'Iter (\d+), learning rates \(--lr_decay \w+, iteration (\d+) of the schedule, factor (\S+)\): D (\S+) G (\S+)'
    assert re.findall(pat, line) == [('3', '7', '0.4', '0.00016', '8e-05')]
