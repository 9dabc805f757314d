"""Autograd surface of the conditional BatchNorm kernels (csrc/pointwise.hip `t2v_cbn_*`), opt-in through
`MultiScaleGen(cond_bn=True)` on the text-conditioned generator (DESIGN "Conditional BatchNorm"; not in the reference).

One definition. Every BatchNorm2d of the generator is a site k with C_k channels, in module registration order. One table per
generator forward, tab = cond · Wᵀ + b [B, 2·ΣC] (`cond_bn.weight`, `cond_bn.bias`; cond is the CA vector c with CA, the sentence
code without); site k owns columns o_k .. o_k + 2·C_k laid out [Δγ (C_k) | Δβ (C_k)], o_k = 2·Σ_{j<k} C_j. A site at pyramid
level ℓ sees x [b_ℓ·T_ℓ, C, H, W]; row n belongs to level sample j = n // T_ℓ, which is base sample j·s (s = 2^ℓ in training
mode, where Subsample keeps ::2; s = 1 in eval mode):

    x̂ = (x − mean_c) · istd_c                            batch statistics over all rows; running stats and counter as BatchNorm2d
    y = x̂ · (γ_c + Δγ[j·s, c]) + (β_c + Δβ[j·s, c])      then the fused ReLU / 2x up-sampling / fork of the site it replaces

Eval mode uses the running statistics and the same per-sample affine. The statistics do not depend on the affine: (mean, 1/std),
the running statistics and num_batches_tracked equal the plain site's on the same x. Adjoint, g' = dL/dy behind the ReLU mask /
up-sampling adjoint, M = rows·H·W, Γ[n,c] = γ_c + Δγ[sample(n)·s, c]:

    sβ[n,c] = Σ_hw g'                          sγ[n,c] = Σ_hw g'·x̂
    dΔβ[j·s,c] = Σ_{n in sample j} sβ[n,c]     dΔγ[j·s,c] = Σ_{n in sample j} sγ[n,c]
    dβ_c = Σ_n sβ    dγ_c = Σ_n sγ             A_c = Σ_n Γ·sβ    B_c = Σ_n Γ·sγ
    dx = istd_c · (Γ·g' − A_c/M − x̂·B_c/M)    (+ the fork's second gradient)

A site's backward writes every row of its own columns of dL/dtab [B, 2·ΣC]: the sums for the rows its level holds, exact zeros
for the others. The buffer therefore needs no fill, no per-site slice gradient is summed by the autograd engine, and the
projection's backward (`table`: the Linear kernels behind `_Table`) consumes the one buffer. How: the first site whose backward
runs allocates the buffer and is the only one that returns it as the table's gradient; the engine runs the table's node after
all 16 sites, by which time every column has been written. First order only; fp32 whatever the convolution precision.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ._ops import _stream, _p, _c, lib, check


class _Shared(object):
    """The dL/dtab buffer the sites of one generator forward share, and how many of them have written their columns."""

    def __init__(self, nsites):
        self.nsites, self.gtab, self.done = nsites, None, 0


class Modulation(object):
    """The table of one generator forward. Handed down through the blocks of that forward; nothing outlives it."""

    def __init__(self, tab, shared):
        self.tab, self.shared = tab, shared

    def site(self, off, s, T):
        """What one BatchNorm site needs: (table, shared state, column offset, base-row stride, frames per sample)."""
        return (self.tab, self.shared, off, s, T)


class _Table(Function):
    """Identity on the table in front of its sites. Its backward receives the ONE dL/dtab buffer and hands it to the projection
    (a Linear); it refuses a backward in which a site did not report (its columns would be unwritten memory)."""

    @staticmethod
    def forward(ctx, tab, shared):
        ctx.shared = shared
        ctx.set_materialize_grads(False)
        return tab.view_as(tab)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        sh = ctx.shared
        if g is None:
            return None, None
        if sh.done != 0 or sh.gtab is None or g.data_ptr() != sh.gtab.data_ptr():
            raise RuntimeError('conditional BatchNorm: %d of %d sites have not run their backward; every rendered level must '
                               'take part in the loss' % (sh.nsites - sh.done, sh.nsites))
        sh.gtab = None
        return g, None


def table(cond, weight, bias, nsites):
    """The per-forward modulation: tab = cond · Wᵀ + b [B, 2·ΣC] in one launch."""
    from . import functional as TF
    shared = _Shared(nsites)
    tab = TF.linear(cond, weight, bias)
    return Modulation(_Table.apply(tab, shared) if tab.requires_grad else tab, shared)


class CondBatchNormAct(Function):
    """One conditional site: `BatchNormAct` / `BatchNormActFork` (functional.py) with the per-sample affine of the table.
    `fork`: returns (y, x') with x' an alias of x for its other consumer, whose gradient joins dL/dx in the backward pass."""

    @staticmethod
    def forward(ctx, x, gamma, beta, tab, rmean, rvar, training, momentum, eps, relu, counter, up, fork, shared, off, s, T):
        x, tab = _c(x), _c(tab)
        if x.dim() != 4:
            raise ValueError('conditional BatchNorm2d takes [N,C,H,W] inputs')
        N, Cc, H, W = x.shape
        R, ld = tab.shape
        ctx.cfg = (bool(up), bool(relu), bool(fork), shared, off, s, T, R, ld)
        ctx.training = training
        shape = (N, Cc, 2 * H, 2 * W) if up else (N, Cc, H, W)
        if training:
            y = torch.empty(shape, device=x.device, dtype=torch.float32)
            stats = torch.empty((2 * Cc,), device=x.device, dtype=torch.float32)
            ws = torch.empty((int(lib().t2v_cbn_ws_floats(N, Cc, H * W)),), device=x.device, dtype=torch.float32)
            fn, name = (lib().t2v_cbn_train_fwd_up, 't2v_cbn_train_fwd_up') if up else (lib().t2v_cbn_train_fwd, 't2v_cbn_train_fwd')
            check(fn(_p(x), _p(gamma), _p(beta), _p(tab), _p(y), _p(stats), _p(rmean), _p(rvar), _p(ws), N, Cc, H, W, ld, off, s, T, R,
                     momentum, eps, int(relu), _p(counter), _stream()), name)
            ctx.save_for_backward(x, y, stats, gamma, tab)
        else:
            y = torch.empty_like(x)
            check(lib().t2v_cbn_eval(_p(x), _p(rmean), _p(rvar), _p(gamma), _p(beta), _p(tab), _p(y), N, Cc, H, W, ld, off, s, T, R,
                                     eps, int(relu), _stream()), 't2v_cbn_eval')
            if up:                  # (sampling path: two launches, like the plain site)
                y2 = torch.empty(shape, device=x.device, dtype=torch.float32)
                check(lib().t2v_upsample2x(_p(y), _p(y2), N * Cc, H, W, _stream()), 't2v_upsample2x')
                y = y2
        ctx.set_materialize_grads(False)
        return (y, x.view_as(x)) if fork else y

    @staticmethod
    @once_differentiable
    def backward(ctx, g, g2=None):
        if not ctx.training:
            raise RuntimeError('eval-mode BatchNorm backward is not on the hot path')
        up, relu, fork, shared, off, s, T, R, ld = ctx.cfg
        x, y, stats, gamma, tab = ctx.saved_tensors
        N, Cc, H, W = x.shape
        first = shared.done == 0
        if first:
            shared.gtab = torch.empty((R, ld), device=x.device, dtype=torch.float32)
        shared.done = (shared.done + 1) % shared.nsites
        gtab = shared.gtab
        if g is None:
            # only the alias was used: the site's columns of dL/dtab are zeros (a [R, 2C] block of the fill kernel, copied in)
            from . import functional as TF
            TF._copy2d(TF.zeros((R, 2 * Cc), x.device), 0, 2 * Cc, gtab, off, ld, R, 2 * Cc)
            return (g2, None, None, gtab if first else None) + (None,) * 13
        g = _c(g)
        g2 = _c(g2) if g2 is not None else None
        gx, gg, gb = torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(gamma)
        ws = torch.empty((int(lib().t2v_cbn_ws_floats(N, Cc, H * W)),), device=x.device, dtype=torch.float32)
        if fork:
            check(lib().t2v_cbn_train_bwd_add(_p(g), _p(x), _p(y), _p(stats), _p(gamma), _p(tab), _p(g2), _p(gx), _p(gg), _p(gb), _p(gtab),
                                              _p(ws), N, Cc, H, W, ld, off, s, T, R, int(up), int(relu), _stream()), 't2v_cbn_train_bwd_add')
        else:
            fn, name = (lib().t2v_cbn_train_bwd_up, 't2v_cbn_train_bwd_up') if up else (lib().t2v_cbn_train_bwd, 't2v_cbn_train_bwd')
            check(fn(_p(g), _p(x), _p(y), _p(stats), _p(gamma), _p(tab), _p(gx), _p(gg), _p(gb), _p(gtab), _p(ws), N, Cc, H, W, ld, off, s,
                     T, R, int(relu), _stream()), name)
        return (gx, gg, gb, gtab if first else None) + (None,) * 13


def cond_batch_norm_act(x, gamma, beta, rmean, rvar, training, mod, momentum=0.1, eps=1e-5, relu=False, counter=None, up=False,
                        fork=False):
    """`functional.batch_norm_act` for a conditional site; `mod` = `Modulation.site(off, s, T)`."""
    tab, shared, off, s, T = mod
    if counter is not None and (counter.dtype != torch.int64 or not counter.is_cuda):
        raise TypeError('num_batches_tracked must be an int64 device tensor')
    forked = bool(fork and training and x.requires_grad and torch.is_grad_enabled())
    out = CondBatchNormAct.apply(x, gamma, beta, tab, rmean, rvar, training, momentum, eps, relu, counter, up, forked, shared, off, s, T)
    if fork and not forked:
        return out, x
    return out
