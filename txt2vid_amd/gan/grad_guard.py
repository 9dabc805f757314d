"""Gradient clipping and a non-finite guard that run inside the replayed graph (opt-in through `--grad_guard`, `--D_clip C`,
`--G_clip C`; the reference has neither). DESIGN §21.

In front of every optimiser step two kinds of launch measure the global L2 norm of the gradients that step is about to read
(after `grad_scale`): `t2v_grad_sumsq_multi` writes one fp32 partial per 4096-element chunk, `t2v_grad_guard` adds them in double
and writes the decision into a float32[8] of device memory per optimiser:

    [0] coef     the factor applied to this step's gradients: min(1, C / (norm + 1e-6)), exactly 1 when nothing is clipped
    [1] skip     1 when the norm is inf or NaN: the step is skipped (parameters, moments and Adam's step counter stay as they are)
    [2] norm     this step's norm
    [3] steps    optimiser steps seen        [4] skipped    steps skipped        [5] clipped    steps with coef < 1

The `_guard` forms of the tick and of the multi-tensor update launches read it at run time, so eager and replayed iterations run
the same launches on the same memory and the decision is taken on the device, per replay. The clipping is
`torch.nn.utils.clip_grad_norm_`'s; the skip departs from torch on purpose (it would scale by NaN)."""
import math

import numpy as np
import torch

from .lr_sched import MAX_UPDATES               # the counts are float32 too: exact below 2^24
CHUNK = 4096                                    # ADAM_CHUNK (csrc/pointwise.hip)
COUNTS = ('steps', 'skipped', 'clipped')


def coef(norm, clip):
    """The host mirror of `t2v_grad_guard`'s coefficient, in the kernel's float32 arithmetic: (coef, skip)."""
    norm = np.float32(norm)
    if not np.isfinite(norm):
        return np.float32(1.0), True
    if clip is None or not clip > 0:
        return np.float32(1.0), False
    c = np.float32(clip) / (norm + np.float32(1e-6))
    return (c if c < np.float32(1.0) else np.float32(1.0)), False


def _clip_value(v, flag):
    if v is None:
        return None
    v = float(v)
    if not (v > 0.0 and math.isfinite(v)):
        raise ValueError('%s takes a finite global-norm bound > 0, got %r' % (flag, v))
    return v


def check_args(args):
    """The rules of --grad_guard / --D_clip / --G_clip: ValueError for a bound that is not a finite positive number,
    NotImplementedError with --end2end; either clip flag implies --grad_guard. Parameter objects without the attributes mean
    "off"."""
    d = _clip_value(getattr(args, 'D_clip', None), '--D_clip')
    g = _clip_value(getattr(args, 'G_clip', None), '--G_clip')
    on = bool(getattr(args, 'grad_guard', False)) or d is not None or g is not None
    if not on:
        return args
    if getattr(args, 'end2end', False):
        raise NotImplementedError('--grad_guard / --D_clip / --G_clip with --end2end: the text encoder sits in both optimisers and '
                                  'its gradients bypass the gradient sink; the guard covers the replayed and the eager GAN loop only')
    spi = max(int(getattr(args, 'discrim_steps', 1)), int(getattr(args, 'gen_steps', 1)), 1)
    iters = getattr(args, 'max_iters', None)
    if iters is not None and int(iters) * spi >= MAX_UPDATES:
        raise ValueError('--max_iters %d with %d optimiser steps per iteration: the device-resident counts of the gradient guard '
                         'are exact below %d steps only' % (iters, spi, MAX_UPDATES))
    args.grad_guard, args.D_clip, args.G_clip = True, d, g
    return args


def enabled(args):
    return bool(getattr(args, 'grad_guard', False)) or getattr(args, 'D_clip', None) is not None or \
        getattr(args, 'G_clip', None) is not None


def n_chunks(numels):
    return sum((int(n) + CHUNK - 1) // CHUNK for n in numels)


class OptGuard(object):
    """One optimiser's side (`optim.Adam.grad_guard` / `optim.SGD.grad_guard`): `state` is the float32[8] the guarded launches
    read, `partials` the per-chunk sums of squares, `measure(jobs, n, gscale)` the launches in front of them."""

    def __init__(self, guard, which, opt):
        self.guard, self.which = guard, which
        self.state, self.clip = guard.state[which], guard.clip[which]
        # one slot per 4096-element chunk of every parameter; a tap-major weight updated by its live taps is one job per tap,
        # each with a chunk count of its own (at most one more per tap)
        slots = 0
        for group in opt.param_groups:
            for p in group['params']:
                taps = 1
                for s in p.shape[2:]:
                    taps *= int(s)
                slots += (p.numel() + CHUNK - 1) // CHUNK + taps
        self.partials = torch.zeros(max(slots, 1), dtype=torch.float32).to(self.state.device)

    def measure(self, jobs, njobs, gscale):
        """sumsq over exactly `jobs` (an AdamJob array), then the decision: ceil(njobs / 64) + 1 launches."""
        from .. import functional as TF
        if not self.state.is_cuda:
            raise RuntimeError('t2v kernels need device tensors: the HIP path has no CPU fallback')
        need = n_chunks(jobs[i].n for i in range(njobs))
        if need > self.partials.numel():
            raise RuntimeError('the gradient guard holds %d chunk sums, this step has %d chunks: attach the guard after the '
                               "optimiser's parameter list is complete" % (self.partials.numel(), need))
        TF.check(TF.lib().t2v_grad_sumsq_multi(jobs, njobs, gscale, TF._p(self.partials), TF._stream()), 't2v_grad_sumsq_multi')
        TF.check(TF.lib().t2v_grad_guard(TF._p(self.partials), need, self.clip or 0.0, TF._p(self.state), TF._stream()),
                 't2v_grad_guard')


class GradGuard(object):
    """The configuration and the two device states. `clip_D` / `clip_G`: the bound on that optimiser's global gradient norm, or
    None (measure and skip non-finite steps only)."""

    def __init__(self, clip_D=None, clip_G=None, device='cpu'):
        self.clip = {'D': _clip_value(clip_D, 'clip_D'), 'G': _clip_value(clip_G, 'clip_G')}
        # made once (by copy: no fill kernel) and only ever written in place: captured graphs keep the addresses
        self.state = {w: torch.tensor([1.0] + [0.0] * 7, dtype=torch.float32).to(device) for w in ('D', 'G')}
        self.opts = {}
        self.slots, self.key = [('guard.' + w, self.state[w], 6) for w in ('D', 'G')], 'grad_guard'       # gan/extras.py

    def attach(self, optD, optG):
        for w, opt in (('D', optD), ('G', optG)):
            opt.grad_guard = OptGuard(self, w, opt)
            self.opts[w] = opt
            if self.state[w].is_cuda:
                # Adam: the device-resident step counter is the one a skipped step leaves alone, so it exists from here on
                # (also for eager runs) and is authoritative
                opt.make_capturable(self.state[w].device)
        return self

    def log_lines(self, iteration, values):
        return [log_line(iteration, unpack(values['guard.D']), unpack(values['guard.G']))] if 'guard.D' in values else []

    def config(self):
        return {'clip_D': self.clip['D'], 'clip_G': self.clip['G']}

    # ---- reads of the device (a host sync, off the hot path) ------------------------------------------------------------------
    def read(self):
        """{'D' | 'G': {coef, skip, norm, steps, skipped, clipped}} of the last optimiser steps."""
        return {w: unpack(self.state[w].tolist()) for w in ('D', 'G')}

    def counters(self):
        r = self.read()
        return {w: {k: r[w][k] for k in COUNTS} for w in ('D', 'G')}

    def state_dict(self):
        sd = self.counters()
        sd['config'] = self.config()
        return sd

    def load_state_dict(self, sd=None):
        """`sd`: a `state_dict()`, or None (a file written without the flags): the counts then start from zero. Returns the lines
        worth reporting; the bounds of this object (the flags) always win."""
        notes = []
        if sd is None:
            counts = {w: dict.fromkeys(COUNTS, 0) for w in ('D', 'G')}
            notes.append('the checkpoint has no grad_guard key: the counts start from zero')
        else:
            counts = {w: {k: int(sd[w][k]) for k in COUNTS} for w in ('D', 'G')}
            saved = sd.get('config')
            if saved is not None and saved != self.config():
                notes.append('the checkpoint was written under other bounds (%s); the flags win (%s)' % (saved, self.config()))
        for w in ('D', 'G'):
            for k in COUNTS:
                if counts[w][k] < 0:
                    raise ValueError('%s count %d of %s is negative' % (k, counts[w][k], w))
            if counts[w]['steps'] >= MAX_UPDATES:
                raise ValueError('%d optimiser steps of %s: the device-resident counts are exact below %d only' % (
                    counts[w]['steps'], w, MAX_UPDATES))
            row = [1.0, 0.0, 0.0] + [float(counts[w][k]) for k in COUNTS] + [0.0, 0.0]
            self.state[w].copy_(torch.tensor(row, dtype=torch.float32))                # in place
        return notes


def unpack(row):
    """The first six floats of a guard state as a dict (counts as ints)."""
    return {'coef': float(row[0]), 'skip': int(row[1]), 'norm': float(row[2]), 'steps': int(round(row[3])),
            'skipped': int(round(row[4])), 'clipped': int(round(row[5]))}


def log_line(iteration, d, g):
    """The line printed at --log_period (`d`, `g`: `unpack`ed states of the last D and G step)."""
    return ('Iter %d, gradient guard: norm D %.6g G %.6g, coef D %.6g G %.6g, skipped D %d G %d, clipped D %d G %d' % (
        iteration, d['norm'], g['norm'], d['coef'], g['coef'], d['skipped'], g['skipped'], d['clipped'], g['clipped']))
