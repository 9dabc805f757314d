"""Autograd surface of the conditioning-augmentation kernels (csrc/pointwise.hip `t2v_ca_fwd` / `t2v_ca_bwd`): StackGAN++'s CA on
the text-conditioned generator's input, opt-in through `MultiScaleGen(ca_dim=D)` (DESIGN "Conditioning augmentation").

    h = CA.fc(s) [B, 4D] -> GLU -> mu, logvar [B, D];  c = mu + eps * exp(logvar / 2);  KL = mean(-0.5 (1 + logvar - mu^2 - e^logvar))

`CondAug` takes h, z and eps and returns (fc_input = [z | c], KL) from ONE launch; its backward is ONE launch whichever of the two
upstream gradients is live. eps carries no gradient (drawn on the host, like z). First-order only: the generator never sits
inside the gradient penalty's double backward. fp32 whatever the convolution precision.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ._ops import _stream, _p, _c, lib, check


class CondAug(Function):
    @staticmethod
    def forward(ctx, h, z, eps, kl_coeff):
        h, z, eps = _c(h), _c(z), _c(eps)
        B, D4 = h.shape
        D, L = D4 // 4, z.shape[1]
        if D4 % 4 or z.shape[0] != B or tuple(eps.shape) != (B, D):
            raise ValueError('conditioning augmentation: h %s, z %s, eps %s do not fit' % (tuple(h.shape), tuple(z.shape),
                                                                                          tuple(eps.shape)))
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(h, eps)
        ctx.cfg = (B, L, D, float(kl_coeff))
        out = torch.empty((B, L + D), device=h.device, dtype=torch.float32)
        kl = torch.empty((), device=h.device, dtype=torch.float32)
        check(lib().t2v_ca_fwd(_p(h), _p(z), _p(eps), _p(out), _p(kl), B, L, D, _stream()), 't2v_ca_fwd')
        return out, kl

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_kl):
        if g_out is None and g_kl is None:
            return None, None, None, None
        h, eps = ctx.saved_tensors
        B, L, D, kl_coeff = ctx.cfg
        gh = torch.empty_like(h)
        check(lib().t2v_ca_bwd(_p(None if g_out is None else _c(g_out)), _p(None if g_kl is None else _c(g_kl)), kl_coeff, _p(h),
                               _p(eps), _p(gh), B, L, D, _stream()), 't2v_ca_bwd')
        return gh, None, None, None


def cond_aug(h, z, eps, kl_coeff=1.0):
    """([z | c] [B, L + D], KL 0-d). `kl_coeff` scales the KL's incoming gradient inside the backward launch; the model passes 1
    (the loss already weights the KL through `scalar_sum`)."""
    return CondAug.apply(h, z, eps, kl_coeff)
