"""Adaptive strength of the discriminator's augmentation (ADA, Karras et al. 2020; opt-in through `--D_ada`, not in the reference;
DESIGN §19): the device-resident controller state and its ONE launch per D step (csrc/diffaug.hip `t2v_ada_update`). The
semantics — gating, the paired overfitting statistic, the controller — are defined once, in txt2vid_amd/functional_aug.py.

    ada float32[8] = {p, sum of sgn(u_r - u_f) in the window, pairs in the window, D steps in the window, 0, 0, 0, 0}

The augmentation launches read p = ada[0] from device memory and `observe` updates it in place, so a replayed HIP graph follows p
without a host sync and without a re-capture. The defaults (target 0.6, interval 4, 500 kclips) are the paper's values for
images; nobody has tuned them for video or for the paired statistic."""
import math

import torch

from .._lib import AdaLevel, MAX_GROUPS

N_STATE = 8


def step_size(batch, interval, kclips):
    """How far p moves per update: B * interval / (1000 * kclips) in double (p crosses [0, 1] in `kclips` thousand clips)."""
    return float(batch) * float(interval) / (1000.0 * float(kclips))


def check_args(args, world=1):
    """The rules of --D_aug_p / --D_ada (ValueError otherwise); resolves `args.D_aug_p` (None: 1.0 without --D_ada, 0.0 with
    it). Parameter objects without the attributes mean "off"."""
    p, target = getattr(args, 'D_aug_p', None), getattr(args, 'D_ada', None)
    if p is None and target is None:
        return args
    if not getattr(args, 'D_aug', ''):
        raise ValueError('--D_aug_p and --D_ada set the strength of --D_aug: give a non-empty --D_aug policy')
    if target is not None:
        if not 0.0 < target < 1.0:
            raise ValueError('--D_ada takes a target in (0, 1) (the paper uses 0.6), got %r' % (target,))
        if getattr(args, 'D_ada_interval', 4) < 1:
            raise ValueError('--D_ada_interval must be >= 1')
        if not getattr(args, 'D_ada_kclips', 500.0) > 0:
            raise ValueError('--D_ada_kclips must be > 0')
        if world > 1:
            raise ValueError('--D_ada in a data-parallel run: every rank would steer its own p from its own window; '
                             'synchronising the window across ranks is not implemented')
    if p is None:
        p = 0.0 if target is not None else 1.0
    if not 0.0 <= p <= 1.0:
        raise ValueError('--D_aug_p takes a probability in [0, 1], got %r' % (p,))
    args.D_aug_p = p
    return args


class AdaState(object):
    """The controller: `target`, `interval` (D steps per update), `kclips` (thousands of clips in which p can cross [0, 1]),
    `p0` (the initial p), and the device state `ada`. `p` is the one-float view the gated augmentation launches read."""

    def __init__(self, target, interval=4, kclips=500.0, p0=0.0, device='cpu'):
        if not 0.0 < float(target) < 1.0:
            raise ValueError('the target of the controller lies in (0, 1), got %r' % (target,))
        if int(interval) < 1 or not float(kclips) > 0 or not 0.0 <= float(p0) <= 1.0:
            raise ValueError('interval >= 1, kclips > 0 and 0 <= p0 <= 1 (got %r, %r, %r)' % (interval, kclips, p0))
        self.target, self.interval, self.kclips, self.p0 = float(target), int(interval), float(kclips), float(p0)
        host = torch.zeros(N_STATE, dtype=torch.float32)
        host[0] = self.p0
        self.ada = host.to(device)                     # (by copy: no fill kernel)
        self.p = self.ada[0:1]
        self.slots, self.key = [('ada.p', self.p, 1)], None            # gan/extras.py: p travels with the losses

    def observe(self, u_r, u_f):
        """One D step's unconditional real / generated logits (a list per pyramid level, or one tensor) into the window, and the
        update of p when the window is full: ONE launch, capturable, no host sync."""
        from .._ops import _stream, _c, lib, check
        if torch.is_tensor(u_r):
            u_r, u_f = [u_r], [u_f]
        if len(u_r) != len(u_f) or not 1 <= len(u_r) <= MAX_GROUPS:
            raise ValueError('1 to %d levels of paired logits, got %d and %d' % (MAX_GROUPS, len(u_r), len(u_f)))
        if not self.ada.is_cuda:
            raise RuntimeError('t2v kernels need device tensors: the HIP path has no CPU fallback')
        rs, fs = [_c(r.detach()) for r in u_r], [_c(f.detach()) for f in u_f]
        arr = (AdaLevel * len(rs))()
        for a, r, f in zip(arr, rs, fs):
            if r.numel() != f.numel() or r.numel() < 1:
                raise ValueError('paired logits: %s against %s' % (tuple(r.shape), tuple(f.shape)))
            a.real, a.fake, a.count = r.data_ptr(), f.data_ptr(), r.numel()
        step = step_size(rs[0].numel(), self.interval, self.kclips)
        if not math.isfinite(step):
            raise ValueError('step %r is not finite' % step)
        check(lib().t2v_ada_update(self.ada.data_ptr(), arr, len(rs), self.target, step, self.interval, _stream()), 't2v_ada_update')

    def log_lines(self, iteration, values):
        return ['Iter %d, augmentation probability p (--D_ada, target %g): %.4f' % (iteration, self.target, p[0])
                for p in [values.get('ada.p')] if p]

    def state_dict(self):
        return {'ada': self.ada.detach().to('cpu', torch.float32).clone()}

    def load_state_dict(self, sd):
        """`sd`: a `state_dict()`; None keeps p0 and an empty window."""
        host = torch.zeros(N_STATE, dtype=torch.float32)
        host[0] = self.p0
        if sd is not None:
            got = sd['ada'].detach().to('cpu', torch.float32).reshape(-1)
            if got.numel() != N_STATE:
                raise ValueError('the controller state is float32[%d], got %d values' % (N_STATE, got.numel()))
            host.copy_(got)
        self.ada.copy_(host)                           # in place: captured graphs keep reading the same address
