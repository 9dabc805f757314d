"""LeCam regularisation of the discriminator (Tseng et al. 2021, "Regularizing Generative Adversarial Networks under Limited
Data"; opt-in through `--D_lecam`, not in the reference): the device-resident anchors and the term's two launches
(csrc/diffaug.hip `t2v_lecam_fwd` / `t2v_lecam_bwd`).

    lecam float32[20] = {n, R_last, gate_last, L, alpha_R[0..7], alpha_F[0..7]}

alpha_R[l] / alpha_F[l] are moving averages of D's unconditional logits of pyramid level l on real / generated clips. One D step,
with n and the anchors as they stood before it:

    gate = n >= max(start, 1)
    R    = 1/L sum_l [ mean_i (u_r[l][i] - alpha_F[l])^2 + mean_i (u_f[l][i] - alpha_R[l])^2 ]        (the paper's plain squares)
    the D loss gains lambda * gate * R; the anchors are constants of differentiation
    alpha <- mean (n == 0), else decay * alpha + (1 - decay) * mean;  n <- n + 1

The forward launch reads and moves the anchors in device memory, so a replayed HIP graph follows them without a host sync and
without a re-capture. lambda = 0.3 is the paper's value for images with hinge-scale logits; nobody has tuned it for video."""
import math

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .._lib import AdaLevel, LecamGrad, MAX_GROUPS

N_STATE = 20
A_R, A_F = 4, 12                # where the anchors of the real / generated logits begin


def check_args(args, world=1):
    """The rules of --D_lecam / --D_lecam_decay / --D_lecam_start (ValueError otherwise). Parameter objects without the
    attributes mean "off"."""
    lam, decay, start = (getattr(args, k, None) for k in ('D_lecam', 'D_lecam_decay', 'D_lecam_start'))
    if lam is None:
        if decay is not None or start is not None:
            raise ValueError('--D_lecam_decay and --D_lecam_start shape --D_lecam: give --D_lecam LAMBDA')
        return args
    if not (float(lam) > 0 and math.isfinite(float(lam))):
        raise ValueError('--D_lecam takes a weight > 0 (the paper uses 0.3), got %r' % (lam,))
    if decay is not None and not 0.0 <= float(decay) < 1.0:
        raise ValueError('--D_lecam_decay takes a decay in [0, 1), got %r' % (decay,))
    if start is not None and (int(start) != start or start < 0):
        raise ValueError('--D_lecam_start counts discriminator steps: an integer >= 0, got %r' % (start,))
    names = getattr(args, 'D_names', None) or getattr(args, 'D', None) or []
    if len(names) > 1:
        raise ValueError('--D_lecam regularises the first and only discriminator, %d are configured' % len(names))
    if world > 1:
        raise ValueError('--D_lecam in a data-parallel run: every rank would keep anchors of its own logits; '
                         'synchronising them across ranks is not implemented')
    args.D_lecam_decay = 0.99 if decay is None else float(decay)
    args.D_lecam_start = 0 if start is None else int(start)
    return args


class _Term(Function):
    """gate * R of one D step (0-d) from the paired logits of every level: ONE launch forward, ONE backward. args: the state
    object, L, u_r[0..L-1], u_f[0..L-1]. The anchors and the gate the forward USED travel to the backward in `saved`, a buffer of
    this call: the forward launch moves the anchors in the state, and under replay the next step's forward has not run yet."""

    @staticmethod
    def forward(ctx, state, L, *us):
        from .._ops import _stream, _c, lib, check
        us = [_c(u) for u in us]
        arr = (AdaLevel * L)()
        for a, r, f in zip(arr, us[:L], us[L:]):
            a.real, a.fake, a.count = r.data_ptr(), f.data_ptr(), r.numel()
        saved = torch.empty(2 * L + 1, device=state.lecam.device, dtype=torch.float32)
        out = torch.empty((), device=state.lecam.device, dtype=torch.float32)
        check(lib().t2v_lecam_fwd(state.lecam.data_ptr(), arr, L, state.decay, state.start, saved.data_ptr(), out.data_ptr(),
                                  _stream()), 't2v_lecam_fwd')
        ctx.L = L
        ctx.save_for_backward(saved, *us)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        from .._ops import _stream, _c, lib, check
        L, (saved, us) = ctx.L, (ctx.saved_tensors[0], ctx.saved_tensors[1:])
        need = ctx.needs_input_grad[2:]
        grads = [torch.empty_like(u) if on else None for u, on in zip(us, need)]
        if any(need):
            g = _c(g)
            arr = (LecamGrad * L)()
            for k, a in enumerate(arr):
                a.real, a.fake, a.count = us[k].data_ptr(), us[L + k].data_ptr(), us[k].numel()
                a.d_real = None if grads[k] is None else grads[k].data_ptr()
                a.d_fake = None if grads[L + k] is None else grads[L + k].data_ptr()
            check(lib().t2v_lecam_bwd(arr, L, saved.data_ptr(), g.data_ptr(), _stream()), 't2v_lecam_bwd')
        return (None, None) + tuple(grads)


class LeCamState(object):
    """The regulariser: `lam` (the weight of the term in the D loss), `decay` of the anchors, `start` (D steps before the term
    counts) and the device state `lecam`."""

    def __init__(self, lam, decay=0.99, start=0, device='cpu'):
        if not (float(lam) > 0 and math.isfinite(float(lam))):
            raise ValueError('the weight of the term is > 0, got %r' % (lam,))
        if not 0.0 <= float(decay) < 1.0 or int(start) < 0:
            raise ValueError('0 <= decay < 1 and start >= 0 (got %r, %r)' % (decay, start))
        self.lam, self.decay, self.start = float(lam), float(decay), int(start)
        self.lecam = torch.zeros(N_STATE, dtype=torch.float32).to(device)      # (by copy: no fill kernel)
        self.slots, self.key = [('lecam', self.lecam, N_STATE)], None          # gan/extras.py: the state travels with the losses

    def term(self, u_r, u_f):
        """gate * R (0-d, differentiable in the logits) of one D step's unconditional real / generated logits (a list per pyramid
        level, or one tensor), and the move of the anchors: ONE launch, capturable, no host sync."""
        if torch.is_tensor(u_r):
            u_r, u_f = [u_r], [u_f]
        u_r, u_f = list(u_r), list(u_f)
        if len(u_r) != len(u_f) or not 1 <= len(u_r) <= MAX_GROUPS:
            raise ValueError('1 to %d levels of paired logits, got %d and %d' % (MAX_GROUPS, len(u_r), len(u_f)))
        if not self.lecam.is_cuda or not all(t.is_cuda for t in u_r + u_f):
            raise RuntimeError('t2v kernels need device tensors: the HIP path has no CPU fallback')
        for r, f in zip(u_r, u_f):
            if r.numel() != f.numel() or r.numel() < 1 or r.dtype != torch.float32 or f.dtype != torch.float32:
                raise ValueError('paired float32 logits: %s against %s' % (tuple(r.shape), tuple(f.shape)))
        return _Term.apply(self, len(u_r), *(u_r + u_f))

    def log_lines(self, iteration, values):
        v = values.get('lecam')
        if not v:
            return []
        L = int(v[3])
        return ['Iter %d, LeCam (--D_lecam %g): R %.6g, gate %d, real %s, fake %s' % (
            iteration, self.lam, v[1], int(v[2]), ' '.join('%.4f' % a for a in v[A_R:A_R + L]),
            ' '.join('%.4f' % a for a in v[A_F:A_F + L]))]

    def state_dict(self):
        return {'lecam': self.lecam.detach().to('cpu', torch.float32).clone()}

    def load_state_dict(self, sd):
        """`sd`: a `state_dict()`; None starts fresh (n = 0, no anchors)."""
        host = torch.zeros(N_STATE, dtype=torch.float32)
        if sd is not None:
            got = sd['lecam'].detach().to('cpu', torch.float32).reshape(-1)
            if got.numel() != N_STATE:
                raise ValueError('the regulariser state is float32[%d], got %d values' % (N_STATE, got.numel()))
            host.copy_(got)
        self.lecam.copy_(host)                         # in place: captured graphs keep reading the same address
