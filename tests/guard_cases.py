"""Shared pieces of the gradient-guard tests (--grad_guard / --D_clip / --G_clip): the float64 statement of the
norm and of torch's clipping coefficient, and the float32 formula the device evaluates."""
import numpy as np
import torch

EPS = 1e-6                                     # torch.nn.utils.clip_grad_norm_'s


def norm64(grads, gscale=1.0):
    """sqrt(sum((gscale * g)^2)) in float64 over CPU copies of the tensors (gscale rounded to float32 as the launch passes it)."""
    s = float(np.float32(gscale))
    return float(torch.sqrt(sum((g.detach().double().cpu() * s).pow(2).sum() for g in grads)))


def torch_coef64(norm, clip):
    """clip_grad_norm_'s coefficient on a float64 norm: clamp(clip / (norm + 1e-6), max=1)."""
    g = torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))
    g.grad = torch.tensor([float(norm)], dtype=torch.float64)
    torch.nn.utils.clip_grad_norm_([g], clip)
    return float(g.grad[0]) / float(norm)


def coef32(norm, clip):
    """The device's formula in float32 on the device's own norm: exactly 1 where C / (norm + 1e-6) >= 1."""
    c = np.float32(clip) / (np.float32(norm) + np.float32(EPS))
    return np.float32(1.0) if c >= np.float32(1.0) else c


def within_one_ulp(a, b):
    a, b = np.float32(a), np.float32(b)
    return a == b or a == np.nextafter(b, np.float32(np.inf)) or a == np.nextafter(b, np.float32(-np.inf))
