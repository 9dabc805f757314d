"""Autograd surface of the contrastive clip-caption matching term (csrc/match.hip `t2v_match_fwd` / `t2v_match_bwd`), opt-in
through `Resnet3D(match=True)` on the text-conditioned discriminator and `--D_match` / `--G_match` (XMC-GAN, Zhang et
al. 2021; not in the reference).

One definition. The head is `match.weight` = W [K, J] (K the trunk's feature width, J = cond_dim). One member has b rows:
features f [b, K] (the trunk's spatially summed features) and sentence codes s [b, J].

    e = f W                            [b, J]
    ê_i = e_i / max(‖e_i‖, 1e-12),   ŝ_j = s_j / max(‖s_j‖, 1e-12)
    S_ij = ⟨ê_i, ŝ_j⟩ / τ
    M_ij = 1 if i == j or row s_i differs from row s_j in any fp32 bit pattern, else 0
    L_i  = −S_ii + log Σ_j M_ij exp(S_ij)      (clip → caption)
    L'_j = −S_jj + log Σ_i M_ij exp(S_ij)      (caption → clip)
    term = (1 / 2b) Σ_i (L_i + L'_i)           (b = 1: exactly 0)

The mask M removes false negatives: a clip that carries the same caption as clip i is no negative for i. Each logsumexp
subtracts its row or column maximum over the unmasked entries (τ = 0.01 overflows fp32 otherwise) and is evaluated as
(max − S_ii) + log Σ, which is exactly 0 when only the diagonal is left. The value for several members (pyramid levels) is the
mean of their terms.

`stats` float32[4] = {the value, clip→caption top-1 accuracy of member 0, caption→clip top-1 accuracy of member 0, the number of
entries M_ij = 0 of member 0 (ordered pairs: one pair of equal captions counts 2)}. Row i is a hit when S_ii > S_ij for every
j ≠ i with M_ij = 1 (a row without competitors is a hit).

The adjoint is first order only (the term sits outside the gradient penalty): with P^r, P^c the masked row and column softmaxes,
C = (P^r + P^c − 2I) / (2bτ), dÊ = g·C·Ŝ (times 1/n for n members), and dE_i = (dÊ_i − ê_i⟨ê_i, dÊ_i⟩) / ‖e_i‖ for
‖e_i‖ > 1e-12, exactly 0 otherwise (`F.normalize`'s Jacobian there is 10¹²·I; a row without a direction gets none). Captions get no gradient: the sentence codes are
constants. The embedding e = f W, df = dE Wᵀ and dW = fᵀ dE are the `cond`, `feat` and `weight` roles of functional_proj.py with g
a vector of ones, so dW goes straight into the gradient sink's slot for W. Members whose features need no gradient are left out
of the backward launches. fp32 whatever the convolution precision; the same bits run to run."""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ._lib import MatchMember, MAX_GROUPS, MATCH_MAX_ROWS, MATCH_MAX_COLS
from ._ops import lib, check, _c, _p, _stream
from .functional_proj import ProjCondG

N_STATS = 4


def _check(es, ss, tau, stats):
    n = len(es)
    if not 1 <= n <= MAX_GROUPS:
        raise ValueError('the matching term takes 1..%d members per launch, got %d' % (MAX_GROUPS, n))
    if len(ss) != n:
        raise ValueError('the matching term needs one tensor per member')
    if not (float(tau) > 0 and float(tau) < float('inf')):
        raise ValueError('the matching term needs a temperature > 0, got %r' % (tau,))
    if not all(t.is_cuda for t in list(es) + list(ss) + [stats]):
        raise RuntimeError('t2v kernels need device tensors: the HIP path has no CPU fallback')
    if stats.dtype != torch.float32 or stats.numel() < N_STATS or not stats.is_contiguous():
        raise ValueError('the matching term writes float32[%d] statistics, got %s of %s' % (N_STATS, tuple(stats.shape), stats.dtype))
    J = es[0].shape[-1]
    for e, s in zip(es, ss):
        if e.dim() != 2 or s.dim() != 2 or tuple(e.shape) != tuple(s.shape) or e.shape[1] != J:
            raise ValueError('matching term: embedded features %s and sentence codes %s do not fit' % (tuple(e.shape), tuple(s.shape)))
        if e.dtype != torch.float32 or s.dtype != torch.float32:
            raise ValueError('matching term: float32 tensors, got %s and %s' % (e.dtype, s.dtype))
        if not 1 <= e.shape[0] <= MATCH_MAX_ROWS or not 1 <= J <= MATCH_MAX_COLS:
            raise ValueError('matching term: 1..%d rows of 1..%d columns per member, got %s' % (MATCH_MAX_ROWS, MATCH_MAX_COLS, tuple(e.shape)))
    return J


def match_fwd_raw(es, ss, tau, stats):
    """(out 0-d, coefs [b, b] per member, norms [2b] per member) of the embedded features `es` and sentence codes `ss`: one launch."""
    es, ss = [_c(t) for t in es], [_c(t) for t in ss]
    J = _check(es, ss, tau, stats)
    dev = es[0].device
    coefs = [torch.empty((e.shape[0], e.shape[0]), device=dev, dtype=torch.float32) for e in es]
    norms = [torch.empty((2 * e.shape[0],), device=dev, dtype=torch.float32) for e in es]
    out = torch.empty((), device=dev, dtype=torch.float32)
    arr = (MatchMember * len(es))()
    for a, e, s, c, nr in zip(arr, es, ss, coefs, norms):
        a.e, a.s, a.coef, a.norms, a.de, a.b = e.data_ptr(), s.data_ptr(), c.data_ptr(), nr.data_ptr(), None, e.shape[0]
    check(lib().t2v_match_fwd(arr, len(es), J, float(tau), _p(stats), _p(out), _stream()), 't2v_match_fwd')
    return out, coefs, norms


def match_bwd_raw(g, es, ss, coefs, norms, scale=None):
    """[dL/de per member] from g = dL/dout (0-d device tensor) and what the forward left: one launch. `scale`: the weight of a
    member's term in out, 1 / (members of the forward launch); default: these members were all of them."""
    es, ss, g = [_c(t) for t in es], [_c(t) for t in ss], _c(g)
    if not 1 <= len(es) <= MAX_GROUPS or not (len(ss) == len(coefs) == len(norms) == len(es)):
        raise ValueError('the matching term needs one tensor per member, 1..%d members' % MAX_GROUPS)
    J = es[0].shape[1]
    des = [torch.empty_like(e) for e in es]
    arr = (MatchMember * len(es))()
    for a, e, s, c, nr, d in zip(arr, es, ss, coefs, norms, des):
        if tuple(c.shape) != (e.shape[0], e.shape[0]) or nr.numel() != 2 * e.shape[0] or tuple(s.shape) != tuple(e.shape) or e.shape[1] != J:
            raise ValueError('matching term: the saved coefficients %s do not fit the member %s' % (tuple(c.shape), tuple(e.shape)))
        a.e, a.s, a.coef, a.norms, a.de, a.b = e.data_ptr(), s.data_ptr(), c.data_ptr(), nr.data_ptr(), d.data_ptr(), e.shape[0]
    check(lib().t2v_match_bwd(arr, len(es), J, 1.0 / len(es) if scale is None else float(scale), _p(g), _stream()), 't2v_match_bwd')
    return des


class MatchG(Function):
    """The mean over n members of the matching term of (e_i, s_i) as a 0-d tensor   —   args: tau, stats, n, e_0.., s_0.."""

    @staticmethod
    def forward(ctx, tau, stats, n, *ts):
        es, ss = [_c(t) for t in ts[:n]], [_c(t) for t in ts[n:]]
        out, coefs, norms = match_fwd_raw(es, ss, tau, stats)
        ctx.n = n
        ctx.save_for_backward(*(es + ss + coefs + norms))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        n, saved = ctx.n, ctx.saved_tensors
        es, ss, coefs, norms = saved[:n], saved[n:2 * n], saved[2 * n:3 * n], saved[3 * n:]
        live = [i for i in range(n) if ctx.needs_input_grad[3 + i]]
        des = [None] * n
        if live and g is not None:
            res = match_bwd_raw(g, [es[i] for i in live], [ss[i] for i in live], [coefs[i] for i in live], [norms[i] for i in live], scale=1.0 / n)
            for i, d in zip(live, res):
                des[i] = d
        return (None, None, None) + tuple(des) + (None,) * n


def match_embedded(es, ss, tau, stats):
    """The term of already embedded features (the kernel pair alone, with its autograd surface)."""
    es, ss = list(es), list(ss)
    _check(es, ss, tau, stats)
    return MatchG.apply(float(tau), stats, len(es), *(es + [s.detach() for s in ss]))


def match_group(W, feats, conds, tau, stats, ones=None):
    """The matching term of up to MAX_GROUPS members that share W: mean_i term(feats[i] @ W, conds[i]; tau) as a 0-d tensor, two
    launches (the embedding of all members, the term). `stats`: a float32[4] device tensor the term's launch fills. `ones`: a
    float32 device vector of ones at least as long as the longest member, made outside any graph capture (`CondMatch` holds one). Without it the cached
    constants of `functional.ones_cached` serve, which must then have been filled for these row counts BEFORE any capture: a
    first use inside a capture would record the fill in the graph. Callers that may run under capture pass `ones`."""
    from . import functional as TF
    feats, conds = list(feats), list(conds)
    n = len(feats)
    if not 1 <= n <= MAX_GROUPS:
        raise ValueError('the matching term takes 1..%d members per launch, got %d' % (MAX_GROUPS, n))
    if len(conds) != n:
        raise ValueError('the matching term needs one tensor per member')
    if not (W.is_cuda and all(t.is_cuda for t in feats + conds)):
        raise RuntimeError('t2v kernels need device tensors: the HIP path has no CPU fallback')
    if W.dim() != 2:
        raise ValueError('matching term: the head is a [K, J] matrix, got %s' % (tuple(W.shape),))
    K, J = W.shape
    for f, s in zip(feats, conds):
        if f.dim() != 2 or s.dim() != 2 or f.shape[1] != K or s.shape[1] != J or f.shape[0] != s.shape[0]:
            raise ValueError('matching term: features %s and condition %s do not fit W %s' % (tuple(f.shape), tuple(s.shape), (K, J)))
        if not 1 <= f.shape[0] <= MATCH_MAX_ROWS or J > MATCH_MAX_COLS:
            raise ValueError('matching term: 1..%d rows of 1..%d columns per member, got %s' % (MATCH_MAX_ROWS, MATCH_MAX_COLS,
                                                                                              tuple(s.shape)))
    if ones is not None and (ones.numel() < max(f.shape[0] for f in feats) or not ones.is_cuda):
        raise ValueError('matching term: the vector of ones is shorter than a member')
    gs = [ones[:f.shape[0]] if ones is not None else TF.ones_cached(f[:, 0]) for f in feats]
    es = ProjCondG.apply(n, W, *(gs + feats))
    # a member whose features need no gradient (and W frozen) is left out of the backward launches: the embedding Function marks
    # all its outputs as differentiable, so say it here (a view, no launch)
    es = [e if (W.requires_grad or f.requires_grad) else e.detach() for e, f in zip(es, feats)]
    return MatchG.apply(float(tau), stats, n, *(es + [s.detach() for s in conds]))
