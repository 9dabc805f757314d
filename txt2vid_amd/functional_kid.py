"""Host surface of the Kernel Inception Distance kernels (csrc/kid.hip `t2v_kid_sums`; DESIGN "KID evaluation"; Bińkowski et al.
2018; not in the reference). Evaluation only: no autograd.

One definition. X (real) and Y (generated) are dense fp32 [n, d] feature matrices on the device, s a block size with n % s == 0
and nb = n / s; rows [b·s, (b+1)·s) of X and of Y form block b. With k(u, v) = (alpha · uᵀv + 1)³

    out[b][0] = Σ_{i≠j in block b} k(x_i, x_j)      out[b][1] = Σ_{i≠j in block b} k(y_i, y_j)      out[b][2] = Σ_{i,j in block b} k(x_i, y_j)

as a float64 device tensor [nb, 3]: fp64 on the matrix pipe, two launches, no atomics, the same bits run to run. `estimate` turns
the sums into the unbiased MMD² of every block, their mean and its standard error, in Python floats on the host."""
import ctypes as C
import math

import torch

from ._ops import lib, check, _c, _p, _stream


def check_sizes(n, d, s):
    if n < 2 or d < 1 or s < 2 or s > n or n % s:
        raise ValueError('KID sums take n >= 2 rows of d >= 1 features in blocks of s >= 2 rows with n %% s == 0, got n = %d, '
                         'd = %d, s = %d' % (n, d, s))


def kid_sums_raw(X, Y, s, alpha, out=None, ws=None):
    """The three Gram sums of every block, float64 [n / s, 3] on the device. `out`, `ws`: buffers to reuse (a dense float64
    [n / s, 3] tensor; a uint8 tensor of at least the queried size)."""
    X, Y = _c(X), _c(Y)
    if X.dim() != 2 or X.shape != Y.shape:
        raise ValueError('KID sums take two [n, d] feature matrices of one shape, got %s and %s' % (tuple(X.shape), tuple(Y.shape)))
    n, d = X.shape
    s = int(s)
    check_sizes(n, d, s)
    L = lib()
    need = int(L.t2v_kid_sums_ws_bytes(n, d, s))
    if need < 1:
        raise ValueError('KID sums: no launch plan for n = %d, d = %d, s = %d' % (n, d, s))
    if ws is None:
        ws = torch.empty((need,), device=X.device, dtype=torch.uint8)
    elif ws.dtype != torch.uint8 or not ws.is_cuda or ws.numel() < need or not ws.is_contiguous() or ws.data_ptr() % 8:
        raise ValueError('KID sums: the workspace is a dense, 8-byte aligned uint8 device tensor of at least %d bytes' % need)
    if out is None:
        out = torch.empty((n // s, 3), device=X.device, dtype=torch.float64)
    elif out.dtype != torch.float64 or tuple(out.shape) != (n // s, 3) or not out.is_contiguous() or not out.is_cuda:
        raise ValueError('KID sums go into a dense float64 [%d, 3] device tensor' % (n // s))
    check(L.t2v_kid_sums(_p(X), _p(Y), n, d, s, C.c_double(float(alpha)), _p(out), _p(ws), _stream()), 't2v_kid_sums')
    return out


def estimate(sums, s):
    """(kid, stderr, per-block values) from the [nb][3] sums (nested lists of Python floats):
    KID_b = S0/(s(s−1)) + S1/(s(s−1)) − 2·S2/s², kid their mean, stderr their sample standard deviation / √nb (None for nb = 1)."""
    ks = [float(r[0]) / (s * (s - 1)) + float(r[1]) / (s * (s - 1)) - 2.0 * float(r[2]) / (s * s) for r in sums]
    nb = len(ks)
    kid = sum(ks) / nb
    if nb < 2:
        return kid, None, ks
    var = sum((k - kid) ** 2 for k in ks) / (nb - 1)
    return kid, math.sqrt(var) / math.sqrt(nb), ks
