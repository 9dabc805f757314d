"""Autograd surface of the projection-head kernels (csrc/proj.hip `t2v_proj_*`), opt-in through `Resnet3D(proj=True)` on the
text-conditioned discriminator (DESIGN "Projection head"; Miyato & Koyama 2018; not in the reference).

One definition. V [K, J] = `proj.weight` (K trunk features, J = cond_dim). With f [b, K] the trunk's spatially summed features,
s [b, J] the sentence code and base [b, 1] the existing head fc(cat(f, s)):

    c[b] = base[b] + Σ_k Σ_j f[b,k] · V[k,j] · s[b,j]

The term is the trilinear form T(g, f, s; V) = Σ_b g[b] Σ_kj f[b,k] V[k,j] s[b,j]. Each derivative of T is T with one index left
free, so four roles — one Function and one kernel launch each, for up to MAX_GROUPS members (pyramid levels, batch halves) that
share V — are closed under differentiation to any order:

    rows    y[b]   = base[b] + Σ_kj f[b,k] V[k,j] s[b,j]       ProjRowsG     adjoints: base ← g;  f ← feat(g, s, V);  s ← cond(g, f, V);  V ← weight(g, f, s)
    feat    F[b,k] = g[b] · Σ_j V[k,j] s[b,j]                  ProjFeatG     with G = dL/dF:   g ← rows(G, s, V);  s ← cond(g, G, V);  V ← weight(g, G, s)
    cond    C[b,j] = g[b] · Σ_k f[b,k] V[k,j]                  ProjCondG     with G = dL/dC:   g ← rows(f, G, V);  f ← feat(g, G, V);  V ← weight(g, f, G)
    weight  W[k,j] = Σ_members Σ_b g[b] f[b,k] s[b,j]          ProjWeightG   with G = dL/dW:   g ← rows(f, s, G);  f ← feat(g, s, G);  s ← cond(g, f, G)

The gradient penalty's `autograd.grad(create_graph=True)` sweep and its second backward therefore stay on these kernels. Members
whose gradient is None are left out of a backward launch; an adjoint nobody needs (`needs_input_grad`) is not launched, and the
weight role is not launched inside `functional.input_grads_only()`. When the gradient sink is armed, the weight role writes or
accumulates straight into V's slot (the kernel's accumulate flag), so the contributions of one step — real‖fake heads,
mismatched-caption heads, the penalty's second backward — are never summed by the autograd engine. fp32 whatever the
convolution precision."""
import torch
from torch.autograd import Function

from ._lib import ProjMember, MAX_GROUPS
from ._ops import lib, check, _c, _p, _stream
from .functional_multi import _live, _fork_some


def _table(n, bs, g=None, f=None, s=None, base=None, out=None):
    arr = (ProjMember * n)()
    for i, a in enumerate(arr):
        a.b = bs[i]
        for key, ts in (('g', g), ('f', f), ('s', s), ('base', base), ('out', out)):
            setattr(a, key, ts[i].data_ptr() if ts is not None and ts[i] is not None else None)
    return arr


def _check_members(n, *lists):
    if not 1 <= n <= MAX_GROUPS:
        raise ValueError('the projection head takes 1..%d members per launch, got %d' % (MAX_GROUPS, n))
    for ts in lists:
        if len(ts) != n:
            raise ValueError('the projection head needs one tensor per member')


def proj_rows_raw(V, fs, ss, bases=None):
    """[base + Σ_kj f V s] as [b, 1] tensors, one launch."""
    V, fs, ss = _c(V), [_c(t) for t in fs], [_c(t) for t in ss]
    bases = [_c(t) for t in bases] if bases is not None else None
    K, J = V.shape
    _check_members(len(fs), ss)
    for f, s in zip(fs, ss):
        if f.dim() != 2 or s.dim() != 2 or f.shape[1] != K or s.shape[1] != J or f.shape[0] != s.shape[0]:
            raise ValueError('projection head: features %s and condition %s do not fit V %s' % (tuple(f.shape), tuple(s.shape), (K, J)))
    if bases is not None:
        _check_members(len(fs), bases)
        for f, b in zip(fs, bases):
            if tuple(b.shape) != (f.shape[0], 1):
                raise ValueError('projection head: the logits it adds to are [b, 1], got %s' % (tuple(b.shape),))
    outs = [torch.empty((f.shape[0], 1), device=f.device, dtype=torch.float32) for f in fs]
    arr = _table(len(fs), [f.shape[0] for f in fs], f=fs, s=ss, base=bases, out=outs)
    check(lib().t2v_proj_rows(arr, len(fs), _p(V), K, J, _stream()), 't2v_proj_rows')
    return outs


def proj_feat_raw(V, gs, ss):
    """[g · (s Vᵀ)] as [b, K] tensors, one launch."""
    V, gs, ss = _c(V), [_c(t) for t in gs], [_c(t) for t in ss]
    K, J = V.shape
    _check_members(len(gs), ss)
    for g, s in zip(gs, ss):
        if s.dim() != 2 or s.shape[1] != J or g.numel() != s.shape[0]:
            raise ValueError('projection head: gradient %s and condition %s do not fit V %s' % (tuple(g.shape), tuple(s.shape), (K, J)))
    outs = [torch.empty((s.shape[0], K), device=s.device, dtype=torch.float32) for s in ss]
    arr = _table(len(gs), [s.shape[0] for s in ss], g=gs, s=ss, out=outs)
    check(lib().t2v_proj_feat(arr, len(gs), _p(V), K, J, _stream()), 't2v_proj_feat')
    return outs


def proj_cond_raw(V, gs, fs):
    """[g · (f V)] as [b, J] tensors, one launch."""
    V, gs, fs = _c(V), [_c(t) for t in gs], [_c(t) for t in fs]
    K, J = V.shape
    _check_members(len(gs), fs)
    for g, f in zip(gs, fs):
        if f.dim() != 2 or f.shape[1] != K or g.numel() != f.shape[0]:
            raise ValueError('projection head: gradient %s and features %s do not fit V %s' % (tuple(g.shape), tuple(f.shape), (K, J)))
    outs = [torch.empty((f.shape[0], J), device=f.device, dtype=torch.float32) for f in fs]
    arr = _table(len(gs), [f.shape[0] for f in fs], g=gs, f=fs, out=outs)
    check(lib().t2v_proj_cond(arr, len(gs), _p(V), K, J, _stream()), 't2v_proj_cond')
    return outs


def proj_weight_raw(gs, fs, ss, out=None, accum=False):
    """Σ_members Σ_b g f ⊗ s as one [K, J] tensor (written into, or added onto, `out` when given), one launch."""
    gs, fs, ss = [_c(t) for t in gs], [_c(t) for t in fs], [_c(t) for t in ss]
    _check_members(len(gs), fs, ss)
    K, J = fs[0].shape[1], ss[0].shape[1]
    for g, f, s in zip(gs, fs, ss):
        if f.dim() != 2 or s.dim() != 2 or f.shape[1] != K or s.shape[1] != J or f.shape[0] != s.shape[0] or g.numel() != f.shape[0]:
            raise ValueError('projection head: members of one weight gradient must share K and J')
    if out is None:
        out = torch.empty((K, J), device=fs[0].device, dtype=torch.float32)
    elif tuple(out.shape) != (K, J) or not out.is_contiguous():
        raise ValueError('projection head: the weight gradient goes into a dense [%d, %d] tensor' % (K, J))
    arr = _table(len(gs), [f.shape[0] for f in fs], g=gs, f=fs, s=ss)
    check(lib().t2v_proj_weight(arr, len(gs), _p(out), K, J, 1 if accum else 0, _stream()), 't2v_proj_weight')
    return out


def _aliases(ts, k):
    """k autograd aliases of every tensor of `ts` for k consumers inside a RECORDED backward (grouped forks: their gradients are
    summed by one launch each, not by the engine); the tensors themselves when nothing is recorded or k < 2."""
    ts = list(ts)
    out = []
    for _ in range(k - 1):
        a, ts = _fork_some(ts)
        out.append(a)
    out.append(ts)
    return out


def _weight_grad(V, gs, fs, ss):
    """dL/dV over the given members: into V's gradient-sink slot when one is armed (None once it accumulated), else a Function."""
    from . import functional as TF
    done, gV = TF._to_sink(V, lambda out, acc: proj_weight_raw(gs, fs, ss, out=out, accum=acc))
    if not done:
        gV = ProjWeightG.apply(len(gs), *(list(gs) + list(fs) + list(ss)))
    return gV


def _want_weight(ctx, idx):
    from . import functional as TF
    return ctx.needs_input_grad[idx] and TF._param_grads_enabled


def _scatter(n, idx, res):
    out = [None] * n
    for i, r in zip(idx, res):
        out[i] = r
    return out


class ProjRowsG(Function):
    """ys[i] = (bases[i] +) Σ_kj fs[i] V ss[i]   —   args: n, has_base, V, f_0.., s_0.., (base_0..)."""

    @staticmethod
    def forward(ctx, n, has_base, V, *ts):
        fs, ss = ts[:n], ts[n:2 * n]
        bases = ts[2 * n:] if has_base else None
        ctx.save_for_backward(V, *fs, *ss)
        ctx.cfg = (n, has_base)
        ctx.set_materialize_grads(False)
        return tuple(proj_rows_raw(V, fs, ss, bases))

    @staticmethod
    def backward(ctx, *gys):
        n, has_base = ctx.cfg
        saved = ctx.saved_tensors
        V, fs, ss = saved[0], saved[1:1 + n], saved[1 + n:]
        none = (None,) * n
        live = _live(gys)
        if not live:
            return (None, None, None) + none + none + (none if has_base else ())
        need = ctx.needs_input_grad
        lf = [i for i in live if need[3 + i]]
        ls = [i for i in live if need[3 + n + i]]
        lb = [i for i in live if has_base and need[3 + 2 * n + i]]
        want_w = _want_weight(ctx, 2)
        uses = [u for u in (lb, lf, ls, live if want_w else []) if u]
        al = iter(_aliases(gys, len(uses)) if len(uses) > 1 else [list(gys)] * len(uses))
        d_b = d_f = d_s = none
        d_V = None
        if lb:
            g = next(al)
            d_b = tuple(_scatter(n, lb, [g[i] for i in lb]))
        if lf:
            g = next(al)
            d_f = tuple(_scatter(n, lf, ProjFeatG.apply(len(lf), V, *([g[i] for i in lf] + [ss[i] for i in lf]))))
        if ls:
            g = next(al)
            d_s = tuple(_scatter(n, ls, ProjCondG.apply(len(ls), V, *([g[i] for i in ls] + [fs[i] for i in ls]))))
        if want_w:
            g = next(al)
            d_V = _weight_grad(V, [g[i] for i in live], [fs[i] for i in live], [ss[i] for i in live])
        return (None, None, d_V) + d_f + d_s + (d_b if has_base else ())


class ProjFeatG(Function):
    """Fs[i] = gs[i] · (ss[i] Vᵀ)   —   args: n, V, g_0.., s_0.."""

    @staticmethod
    def forward(ctx, n, V, *ts):
        gs, ss = ts[:n], ts[n:]
        ctx.save_for_backward(V, *ts)
        ctx.n = n
        ctx.set_materialize_grads(False)
        return tuple(proj_feat_raw(V, gs, ss))

    @staticmethod
    def backward(ctx, *GFs):
        n = ctx.n
        saved = ctx.saved_tensors
        V, gs, ss = saved[0], saved[1:1 + n], saved[1 + n:]
        none = (None,) * n
        live = _live(GFs)
        if not live:
            return (None, None) + none + none
        need = ctx.needs_input_grad
        lg = [i for i in live if need[2 + i]]
        ls = [i for i in live if need[2 + n + i]]
        want_w = _want_weight(ctx, 1)
        uses = [u for u in (lg, ls, live if want_w else []) if u]
        al = iter(_aliases(GFs, len(uses)) if len(uses) > 1 else [list(GFs)] * len(uses))
        d_g = d_s = none
        d_V = None
        if lg:
            G = next(al)
            res = _scatter(n, lg, ProjRowsG.apply(len(lg), False, V, *([G[i] for i in lg] + [ss[i] for i in lg])))
            d_g = tuple(None if r is None else r.view_as(gs[i]) for i, r in enumerate(res))
        if ls:
            G = next(al)
            d_s = tuple(_scatter(n, ls, ProjCondG.apply(len(ls), V, *([gs[i] for i in ls] + [G[i] for i in ls]))))
        if want_w:
            G = next(al)
            d_V = _weight_grad(V, [gs[i] for i in live], [G[i] for i in live], [ss[i] for i in live])
        return (None, d_V) + d_g + d_s


class ProjCondG(Function):
    """Cs[i] = gs[i] · (fs[i] V)   —   args: n, V, g_0.., f_0.."""

    @staticmethod
    def forward(ctx, n, V, *ts):
        gs, fs = ts[:n], ts[n:]
        ctx.save_for_backward(V, *ts)
        ctx.n = n
        ctx.set_materialize_grads(False)
        return tuple(proj_cond_raw(V, gs, fs))

    @staticmethod
    def backward(ctx, *GCs):
        n = ctx.n
        saved = ctx.saved_tensors
        V, gs, fs = saved[0], saved[1:1 + n], saved[1 + n:]
        none = (None,) * n
        live = _live(GCs)
        if not live:
            return (None, None) + none + none
        need = ctx.needs_input_grad
        lg = [i for i in live if need[2 + i]]
        lf = [i for i in live if need[2 + n + i]]
        want_w = _want_weight(ctx, 1)
        uses = [u for u in (lg, lf, live if want_w else []) if u]
        al = iter(_aliases(GCs, len(uses)) if len(uses) > 1 else [list(GCs)] * len(uses))
        d_g = d_f = none
        d_V = None
        if lg:
            G = next(al)
            res = _scatter(n, lg, ProjRowsG.apply(len(lg), False, V, *([fs[i] for i in lg] + [G[i] for i in lg])))
            d_g = tuple(None if r is None else r.view_as(gs[i]) for i, r in enumerate(res))
        if lf:
            G = next(al)
            d_f = tuple(_scatter(n, lf, ProjFeatG.apply(len(lf), V, *([gs[i] for i in lf] + [G[i] for i in lf]))))
        if want_w:
            G = next(al)
            d_V = _weight_grad(V, [gs[i] for i in live], [fs[i] for i in live], [G[i] for i in live])
        return (None, d_V) + d_g + d_f


class ProjWeightG(Function):
    """W = Σ_i Σ_b gs[i] fs[i] ⊗ ss[i]   —   args: n, g_0.., f_0.., s_0.."""

    @staticmethod
    def forward(ctx, n, *ts):
        ctx.save_for_backward(*ts)
        ctx.n = n
        ctx.set_materialize_grads(False)
        return proj_weight_raw(ts[:n], ts[n:2 * n], ts[2 * n:])

    @staticmethod
    def backward(ctx, GW):
        n = ctx.n
        saved = ctx.saved_tensors
        gs, fs, ss = saved[:n], saved[n:2 * n], saved[2 * n:]
        none = (None,) * n
        if GW is None:
            return (None,) + none + none + none
        need = ctx.needs_input_grad
        lg = [i for i in range(n) if need[1 + i]]
        lf = [i for i in range(n) if need[1 + n + i]]
        ls = [i for i in range(n) if need[1 + 2 * n + i]]
        uses = [u for u in (lg, lf, ls) if u]
        al = iter(_aliases([GW], len(uses)) if len(uses) > 1 else [[GW]] * len(uses))
        d_g = d_f = d_s = none
        if lg:
            G = next(al)[0]
            res = _scatter(n, lg, ProjRowsG.apply(len(lg), False, G, *([fs[i] for i in lg] + [ss[i] for i in lg])))
            d_g = tuple(None if r is None else r.view_as(gs[i]) for i, r in enumerate(res))
        if lf:
            G = next(al)[0]
            d_f = tuple(_scatter(n, lf, ProjFeatG.apply(len(lf), G, *([gs[i] for i in lf] + [ss[i] for i in lf]))))
        if ls:
            G = next(al)[0]
            d_s = tuple(_scatter(n, ls, ProjCondG.apply(len(ls), G, *([gs[i] for i in ls] + [fs[i] for i in ls]))))
        return (None,) + d_g + d_f + d_s


def proj_rows_group(V, fs, ss, bases=None):
    """[base + ((f @ V) * s).sum(1, keepdim=True) for f, s, base in zip(fs, ss, bases)] in ONE launch: the projection term of the
    conditional heads of up to MAX_GROUPS members that share V, added onto the existing head's logits [b, 1]."""
    fs, ss = list(fs), list(ss)
    _check_members(len(fs), ss)
    if bases is None:
        return list(ProjRowsG.apply(len(fs), False, V, *(fs + ss)))
    bases = list(bases)
    _check_members(len(fs), bases)
    return list(ProjRowsG.apply(len(fs), True, V, *(fs + ss + bases)))
