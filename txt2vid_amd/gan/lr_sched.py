"""Learning-rate decay that runs inside the replayed graph (opt-in through `--lr_decay`; the reference has no schedule, TGANv2's
recipe decays Adam's rate linearly to zero). DESIGN §20.

For the 0-based training iteration `it`, with S = --lr_decay_start, T = --lr_decay_iters, F = --lr_final:

    frac   = clamp((it - S) / (T - S), 0, 1)
    linear : factor = 1 - (1 - F) * frac
    cosine : factor = F + (1 - F) * 0.5 * (1 + cos(pi * frac))
    factor == 1 exactly while frac == 0, and == F exactly once frac == 1

Both optimisers scale their base rate by the factor of the iteration they are in. A captured HIP graph freezes every host float in
its kernel nodes, so the factor lives in device memory: each optimiser owns a float32[2] state {k, factor}, k = its updates so far.
`t2v_lr_tick` in front of every optimiser step writes the factor of iteration k // spi (spi = that optimiser's updates per
iteration: --discrim_steps for D, --gen_steps for G) and advances k; the `_sched` forms of the multi-tensor launches read it. Eager
and replayed iterations run the same launches on the same memory. `param_groups[i]['lr']` keeps the base rate."""
import math

import torch

KINDS = {'linear': 1, 'cosine': 2}             # T2V_LR_LINEAR / T2V_LR_COSINE (include/t2v_hip.h)
MAX_UPDATES = 2 ** 24                          # k is a float32 (like Adam's device-resident step): exact up to here


def factor(kind, it, start, end, final):
    """The schedule in float64 — the host mirror of `t2v_lr_tick`'s arithmetic (it logs the rates; tests/lr_cases.py restates it)."""
    frac = (float(it) - float(start)) / (float(end) - float(start))
    if not frac > 0.0:
        return 1.0
    if frac >= 1.0:
        return float(final)
    if kind == 'linear':
        return 1.0 - (1.0 - float(final)) * frac
    if kind == 'cosine':
        return float(final) + (1.0 - float(final)) * 0.5 * (1.0 + math.cos(math.pi * frac))
    raise ValueError('unknown schedule %r (one of %s)' % (kind, ', '.join(sorted(KINDS))))


def check_args(args):
    """The rules of --lr_decay / --lr_decay_iters / --lr_decay_start / --lr_final (ValueError otherwise); resolves the defaults
    of the last two (0 and 0.0) when a decay is on. Parameter objects without the attributes mean "off"."""
    kind = getattr(args, 'lr_decay', 'none') or 'none'
    T, S, F = (getattr(args, k, None) for k in ('lr_decay_iters', 'lr_decay_start', 'lr_final'))
    if kind == 'none':
        given = [n for n, v in (('--lr_decay_iters', T), ('--lr_decay_start', S), ('--lr_final', F)) if v is not None]
        if given:
            raise ValueError('%s without --lr_decay: name the schedule (linear or cosine)' % ', '.join(given))
        return args
    if kind not in KINDS:
        raise ValueError('--lr_decay takes none, linear or cosine, got %r' % (kind,))
    if T is None:
        raise ValueError('--lr_decay %s needs --lr_decay_iters (the iteration at which the decay ends)' % kind)
    S = 0 if S is None else S
    F = 0.0 if F is None else F
    if S < 0:
        raise ValueError('--lr_decay_start must be >= 0, got %r' % (S,))
    if T <= S:
        raise ValueError('--lr_decay_iters (%r) must lie behind --lr_decay_start (%r)' % (T, S))
    if not 0.0 <= F <= 1.0:
        raise ValueError('--lr_final is the fraction of the base rate that remains, in [0, 1], got %r' % (F,))
    spi = max(int(getattr(args, 'discrim_steps', 1)), int(getattr(args, 'gen_steps', 1)), 1)
    if T * spi >= MAX_UPDATES:
        raise ValueError('--lr_decay_iters %d with %d optimiser steps per iteration: the device-resident update count is exact '
                         'below %d updates only' % (T, spi, MAX_UPDATES))
    args.lr_decay_start, args.lr_final = int(S), float(F)
    return args


class OptSchedule(object):
    """One optimiser's side of the schedule (`optim.Adam.lr_sched` / `optim.SGD.lr_sched`): `state` is the float32[2] {k, factor}
    the scheduled launches read, `tick()` the ONE launch in front of them."""

    def __init__(self, sched, which):
        self.sched, self.which = sched, which
        self.state, self.spi = sched.state[which], sched.spi[which]

    def tick(self):
        from .. import functional as TF
        s = self.sched
        if not self.state.is_cuda:
            raise RuntimeError('t2v kernels need device tensors: the HIP path has no CPU fallback')
        TF.check(TF.lib().t2v_lr_tick(TF._p(self.state), KINDS[s.kind], s.start, s.end, s.final, self.spi, TF._stream()), 't2v_lr_tick')


class LrSchedule(object):
    """The configuration, the two device states and the host mirror. `n_d` / `n_g`: optimiser steps per iteration of D and G."""

    slots, key = (), 'lr_sched'          # gan/extras.py: nothing to read with the losses; the checkpoint key

    def __init__(self, kind, end, start=0, final=0.0, n_d=1, n_g=1, device='cpu'):
        if kind not in KINDS:
            raise ValueError('unknown schedule %r (one of %s)' % (kind, ', '.join(sorted(KINDS))))
        start, end, final, n_d, n_g = int(start), int(end), float(final), int(n_d), int(n_g)
        if start < 0 or end <= start or not 0.0 <= final <= 1.0 or n_d < 1 or n_g < 1:
            raise ValueError('0 <= start < end, 0 <= final <= 1 and at least one step per iteration (got %r, %r, %r, %r, %r)'
                             % (start, end, final, n_d, n_g))
        if end * max(n_d, n_g) >= MAX_UPDATES:
            raise ValueError('the device-resident update count is exact below %d updates only' % MAX_UPDATES)
        self.kind, self.start, self.end, self.final = kind, start, end, final
        self.spi = {'D': n_d, 'G': n_g}
        # {k, factor}, made once (by copy: no fill kernel) and only ever written in place: captured graphs keep the addresses
        self.state = {w: torch.tensor([0.0, 1.0], dtype=torch.float32).to(device) for w in ('D', 'G')}

    def attach(self, optD, optG):
        optD.lr_sched, optG.lr_sched = OptSchedule(self, 'D'), OptSchedule(self, 'G')
        self.opts, self.it0 = {'D': optD, 'G': optG}, 0     # (it0: set when train() starts, extras.training_extras)
        return self

    def log_lines(self, iteration, values):
        it = self.it0 + iteration - 1
        f = self.factor(it)                                    # the host mirror of the formula: nothing is read from the device
        return ['Iter %d, learning rates (--lr_decay %s, iteration %d of the schedule, factor %.6g): D %.6g G %.6g' % (
            iteration, self.kind, it + 1, f, self.opts['D'].param_groups[0]['lr'] * f, self.opts['G'].param_groups[0]['lr'] * f)]

    # ---- host mirror ---------------------------------------------------------------------------------------------------------
    def factor(self, it):
        return factor(self.kind, it, self.start, self.end, self.final)

    def config(self):
        return {'kind': self.kind, 'start': self.start, 'end': self.end, 'final': self.final, 'spi': dict(self.spi)}

    # ---- checkpoints (read the device: a host sync, off the hot path) ----------------------------------------------------------
    def counters(self):
        return {w: int(round(float(self.state[w][0].item()))) for w in ('D', 'G')}

    def state_dict(self):
        sd = self.counters()
        sd['config'] = self.config()
        return sd

    def load_state_dict(self, sd=None, iteration=0):
        """`sd`: a `state_dict()`, or None (a file written without the flag, or by the reference): the counters then start from
        `iteration` * spi. Returns the lines worth reporting; the configuration of this object (the flags) always wins."""
        notes = []
        if sd is None:
            k = {w: int(iteration) * self.spi[w] for w in ('D', 'G')}
            if iteration:
                notes.append('the checkpoint has no lr_sched key: the schedule starts from its iteration %d (D at update %d, G at '
                             'update %d)' % (iteration, k['D'], k['G']))
        else:
            k = {w: int(sd[w]) for w in ('D', 'G')}
            saved = sd.get('config')
            if saved is not None and saved != self.config():
                notes.append('the checkpoint was written under another schedule (%s); the flags win (%s)' % (saved, self.config()))
        for w in ('D', 'G'):
            if k[w] < 0:
                raise ValueError('update count %d of %s is negative' % (k[w], w))
            # in place; a float32 count stops at 2^24, far behind the end of any schedule this object accepts
            self.state[w].copy_(torch.tensor([float(min(k[w], MAX_UPDATES)), 1.0], dtype=torch.float32))
        return notes
