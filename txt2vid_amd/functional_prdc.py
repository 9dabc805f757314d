"""Host surface of the nearest-neighbour kernels behind improved precision/recall (Kynkäänniemi et al. 2019) and density/coverage
(Naeem et al. 2020) (csrc/prdc.hip `t2v_knn_radii`, `t2v_prdc_counts`; DESIGN "Precision/recall and density/coverage"; not in the
reference). Evaluation only: no autograd.

One definition: include/t2v_hip.h. X (real) and Y (generated) are dense fp32 [n, d] feature matrices on the device, 1 <= k <= 16,
k < n; D2(u, v) = max(0, ‖u‖² + ‖v‖² − 2 uᵀv); a radius is the k-th smallest D2 of a row to the OTHER rows of its own bank (squared,
self excluded by index); the four counts c[0..3] are precision·n, density·k·n, recall·n and coverage·n. fp64 on the matrix pipe,
no n x n matrix in memory, the same bits run to run. `estimate` does the four divisions in Python floats on the host."""
import torch

from ._ops import lib, check, _c, _p, _stream

MAX_K = 16                                # T2V_KNN_MAX_K


def check_sizes(n, d, k):
    if n < 2 or d < 1 or k < 1 or k > MAX_K or k >= n:
        raise ValueError('PRDC takes n >= 2 rows of d >= 1 features and 1 <= k <= %d neighbours with k < n, got n = %d, d = %d, '
                         'k = %d' % (MAX_K, n, d, k))


def _workspace(what, query, n, d, k, ws, device):
    need = int(query(n, d, k))
    if need < 1:
        raise ValueError('%s: no launch plan for n = %d, d = %d, k = %d' % (what, n, d, k))
    if ws is None:
        return torch.empty((need,), device=device, dtype=torch.uint8)
    if ws.dtype != torch.uint8 or not ws.is_cuda or ws.numel() < need or not ws.is_contiguous() or ws.data_ptr() % 8:
        raise ValueError('%s: the workspace is a dense, 8-byte aligned uint8 device tensor of at least %d bytes' % (what, need))
    return ws


def _radii(what, r, n):
    if r.dtype != torch.float64 or tuple(r.shape) != (n,) or not r.is_contiguous() or not r.is_cuda:
        raise ValueError('PRDC: %s is a dense float64 [%d] device tensor' % (what, n))
    return r


def knn_radii_raw(U, k, out=None, ws=None):
    """The squared k-th-neighbour radius of every row of U within U, float64 [n] on the device. `out`, `ws`: buffers to reuse (a
    dense float64 [n] tensor; a uint8 tensor of at least the queried size)."""
    U = _c(U)
    if U.dim() != 2:
        raise ValueError('PRDC radii take one [n, d] feature matrix, got %s' % (tuple(U.shape),))
    n, d = U.shape
    k = int(k)
    check_sizes(n, d, k)
    L = lib()
    ws = _workspace('PRDC radii', L.t2v_knn_radii_ws_bytes, n, d, k, ws, U.device)
    out = torch.empty((n,), device=U.device, dtype=torch.float64) if out is None else _radii('the output', out, n)
    check(L.t2v_knn_radii(_p(U), n, d, k, _p(out), _p(ws), _stream()), 't2v_knn_radii')
    return out


def prdc_counts_raw(X, Y, k, rX, rY, out=None, ws=None):
    """The four counts, int64 [4] on the device, from both banks and their radii (`knn_radii_raw` of X and of Y at the same k).
    `out`, `ws`: buffers to reuse (a dense int64 [4] tensor; a uint8 tensor of at least the queried size)."""
    X, Y = _c(X), _c(Y)
    if X.dim() != 2 or X.shape != Y.shape:
        raise ValueError('PRDC counts take two [n, d] feature matrices of one shape, got %s and %s' % (tuple(X.shape), tuple(Y.shape)))
    n, d = X.shape
    k = int(k)
    check_sizes(n, d, k)
    rX, rY = _radii('rX', rX, n), _radii('rY', rY, n)
    L = lib()
    ws = _workspace('PRDC counts', L.t2v_prdc_counts_ws_bytes, n, d, k, ws, X.device)
    if out is None:
        out = torch.empty((4,), device=X.device, dtype=torch.int64)
    elif out.dtype != torch.int64 or tuple(out.shape) != (4,) or not out.is_contiguous() or not out.is_cuda:
        raise ValueError('PRDC counts go into a dense int64 [4] device tensor')
    check(L.t2v_prdc_counts(_p(X), _p(Y), n, d, k, _p(rX), _p(rY), _p(out), _p(ws), _stream()), 't2v_prdc_counts')
    return out


def estimate(counts, n, k):
    """(precision, recall, density, coverage) from the four integer counts: c0/n, c2/n, c1/(k·n), c3/n, in Python floats."""
    c = [int(v) for v in counts]
    n, k = int(n), int(k)
    return c[0] / n, c[2] / n, c[1] / (k * n), c[3] / n
