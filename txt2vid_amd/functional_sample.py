"""Host surface of the sampling tool's two device passes (csrc/sample.hip `t2v_clip_export`, `t2v_clip_nn`; not in the
reference). Evaluation only: no autograd.

One definition: include/t2v_hip.h. `clip_export` turns float clips [B,C,T,H,W] into the frame cache's bytes [B*T, C*H*W] with
q = rint(x * 127.5 + 127.5) in two rounded fp32 operations, clamped, NaN -> 0: `byte_map` below is the same expression in numpy,
bit for bit, and the exact inverse of `data.unit_range`. `clip_nn` merges the squared pixel distances of N samples to one batch of
B real clips into each sample's K nearest so far, ordered by (distance, index); `nn_merge` is that merge in numpy."""
import numpy as np
import torch

from ._ops import lib, check, _c, _p, _stream

NN_MAX_ROWS = 64                          # T2V_CLIP_NN_MAX_ROWS
NN_MAX_K = 8                              # T2V_CLIP_NN_MAX_K
BYTE_MAP = 'u8 = clamp(rint(x * 127.5 + 127.5), 0, 255) in float32, the product and the sum rounded apart, half to even, NaN -> 0; ' \
           'the inverse is data.unit_range: x = (u8 / 255 - 0.5) / 0.5'


def byte_map(x):
    """numpy's float32 expression of the export byte (any shape; no layout change): the kernel's reference, bit for bit."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        q = np.rint(x * np.float32(127.5) + np.float32(127.5))
        q = np.where(np.isnan(q), np.float32(0), np.clip(q, np.float32(0), np.float32(255)))
    return q.astype(np.uint8)


def export_rows(a):
    """[B,C,T,H,W] -> [B*T, C*H*W]: the frame cache's block layout of a channel-first batch (numpy, any dtype)."""
    a = np.asarray(a)
    B, C, T, H, W = a.shape
    return np.ascontiguousarray(a.transpose(0, 2, 1, 3, 4)).reshape(B * T, C * H * W)


def clip_export(x, out=None):
    """uint8 [B*T, C*H*W] on the device from float32 [B,C,T,H,W] (`t2v_clip_export`). `out`: a dense buffer to reuse."""
    x = _c(x)
    if x.dim() != 5:
        raise ValueError('clip_export takes [B,C,T,H,W] clips, got %s' % (tuple(x.shape),))
    B, C, T, H, W = [int(v) for v in x.shape]
    if out is None:
        out = torch.empty((B * T, C * H * W), device=x.device, dtype=torch.uint8)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (B * T, C * H * W) or not out.is_contiguous() or not out.is_cuda:
        raise ValueError('clip_export: the output is a dense uint8 [%d, %d] device tensor' % (B * T, C * H * W))
    check(lib().t2v_clip_export(_p(x), B, C, T, H, W, _p(out), _stream()), 't2v_clip_export')
    return out


def nn_chain(D):
    """The longest chain of fp32 additions behind one returned distance; also the slab length: D is cut into ceil(D / chain) slabs."""
    L = int(lib().t2v_clip_nn_chain(int(D)))
    if L < 1:
        raise ValueError('clip_nn takes D % 4 == 0 with 4 <= D <= 3*16*128*128, got %d' % D)
    return L


def nn_slabs(D):
    return -(-int(D) // nn_chain(D))


def nn_gamma(D):
    """The relative error bound of one distance against the exact sum over the same fp32 inputs: (1 + 2^-24)^(L+2) - 1 for the
    fp32 chain (one rounding of the difference counts twice in its square, one per fma) plus 2^-53 per slab for the fp64 adds."""
    return (1.0 + 2.0 ** -24) ** (nn_chain(D) + 2) - 1.0 + nn_slabs(D) * 2.0 ** -53


def nn_init(N, K, device):
    """The empty lists: (+inf, -1) everywhere."""
    return (torch.full((N, K), float('inf'), dtype=torch.float64).to(device), torch.full((N, K), -1, dtype=torch.int64).to(device))


def check_nn_sizes(N, B, D, K):
    if not (1 <= N <= NN_MAX_ROWS and 1 <= B <= NN_MAX_ROWS and 1 <= K <= NN_MAX_K):
        raise ValueError('clip_nn takes 1..%d samples, 1..%d real clips per call and 1..%d neighbours, got N = %d, B = %d, K = %d'
                         % (NN_MAX_ROWS, NN_MAX_ROWS, NN_MAX_K, N, B, K))
    if int(lib().t2v_clip_nn_ws_bytes(N, B, int(D))) < 1:
        raise ValueError('clip_nn: no plan for D = %d (D %% 4 == 0, 4 <= D <= 3*16*128*128)' % D)


def clip_nn(g, r, base, best_d2, best_idx, ws=None):
    """Merge the candidates (d2(n, j), base + j) of one batch r [B, D] into the lists of the samples g [N, D], in place
    (`t2v_clip_nn`). best_d2 float64 [N, K], best_idx int64 [N, K] (`nn_init`); `ws`: a uint8 buffer to reuse."""
    g, r = _c(g), _c(r)
    if g.dim() != 2 or r.dim() != 2 or g.shape[1] != r.shape[1]:
        raise ValueError('clip_nn takes g [N, D] and r [B, D], got %s and %s' % (tuple(g.shape), tuple(r.shape)))
    N, D = [int(v) for v in g.shape]
    B = int(r.shape[0])
    if best_d2.dim() != 2 or best_d2.shape != best_idx.shape or best_d2.shape[0] != N or best_d2.dtype != torch.float64 or \
            best_idx.dtype != torch.int64 or not best_d2.is_cuda or not best_idx.is_cuda or not best_d2.is_contiguous() or \
            not best_idx.is_contiguous():
        raise ValueError('clip_nn: the lists are dense float64 / int64 [N, K] device tensors')
    K = int(best_d2.shape[1])
    check_nn_sizes(N, B, D, K)
    need = int(lib().t2v_clip_nn_ws_bytes(N, B, D))
    if ws is None:
        ws = torch.empty((need,), device=g.device, dtype=torch.uint8)
    elif ws.dtype != torch.uint8 or not ws.is_cuda or ws.numel() < need or not ws.is_contiguous() or ws.data_ptr() % 4:
        raise ValueError('clip_nn: the workspace is a dense, 4-byte aligned uint8 device tensor of at least %d bytes' % need)
    check(lib().t2v_clip_nn(_p(g), N, _p(r), B, D, int(base), K, _p(best_d2), _p(best_idx), _p(ws), _stream()), 't2v_clip_nn')
    return best_d2, best_idx


def nn_merge(best_d2, best_idx, d2, base):
    """The merge in numpy: best_d2 / best_idx [N, K] ascending by (distance, index), d2 [N, B] the candidates of indices
    base .. base + B - 1. Returns new arrays; NaN candidates are dropped."""
    best_d2, best_idx, d2 = np.asarray(best_d2, np.float64), np.asarray(best_idx, np.int64), np.asarray(d2, np.float64)
    N, K = best_d2.shape
    out_d, out_i = np.empty_like(best_d2), np.empty_like(best_idx)
    for n in range(N):
        cand = [(float(d), int(i)) for d, i in zip(best_d2[n], best_idx[n]) if i >= 0]
        cand += [(float(d), int(base) + j) for j, d in enumerate(d2[n]) if not np.isnan(d) and d < np.inf]
        cand.sort()
        cand = (cand + [(np.inf, -1)] * K)[:K]
        out_d[n], out_i[n] = [c[0] for c in cand], [c[1] for c in cand]
    return out_d, out_i
