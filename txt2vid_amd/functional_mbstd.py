"""Autograd surface of the minibatch-standard-deviation kernels (csrc/mbstd.hip `t2v_mbstd_*`), opt-in through
`Resnet3D(mbstd=G)` on either discriminator (DESIGN "Minibatch standard deviation"; Karras et al. 2018, StyleGAN2's
`MinibatchStdLayer`; not in the reference).

One definition. f [b, K] = the trunk's spatially summed features of one member, with a segment length seg (b % seg == 0, seg = b
unless stated): rows [i·seg, (i+1)·seg) form a segment, consecutive runs of G rows inside a segment a group; the last group of a
segment holds the remainder (possibly one row); groups never cross a segment boundary. Per group q of n rows:

    μ_k = (1/n) Σ_b f_bk      v_k = (1/n) Σ_b (f_bk − μ_k)²      σ_k = sqrt(v_k + 1e-8)      s_q = (1/K) Σ_k σ_k
    y_h[b] = base_h[b] + w_h · s_q(b)               h = 0 the unconditional logit, h = 1 the conditional one; w = `mbstd.weight`

With a_q = Σ_{b∈q} Σ_h g_h[b] w_h, four roles — one Function and one launch each, for up to MAX_GROUPS members that share w:

    fwd     y_h = base_h + w_h s, and s per row       MbstdFwdG      adjoints: base_h ← g_h;  f ← feat(g, f, w);  w ← weight(g, s)
    feat    F_bk = a_q (f_bk − μ_k) / (n K σ_k)       MbstdFeatG     with Γ = dL/dF:  (f, g_h, t) ← second(Γ, g, f, w);  w ← weight(g, t)
    second  t_q = Σ_bk Γ_bk (f_bk − μ_k)/(n K σ_k);  g_h ← w_h t_q;
            f_bk ← (a_q/(nK)) [ (Γ_bk − Γ̄_k)/σ_k − (f_bk − μ_k) Σ_b' Γ_b'k (f_b'k − μ_k)/(n σ_k³) ]       MbstdSecondG   (not differentiable)
    weight  W_h = Σ_members Σ_b g_h[b] stat[b]        MbstdWeightG   (not differentiable)

The gradient penalty's `autograd.grad(create_graph=True)` sweep records `feat`, and its second backward runs `second`: that is
the order training needs, and the two Functions without a written backward raise when they are differentiated. Members whose
gradient is None are left out of a backward launch; an adjoint nobody needs (`needs_input_grad`) is not launched, and the weight
role is not launched inside `functional.input_grads_only()` or with a frozen w. When the gradient sink is armed, the weight role
writes or accumulates straight into w's slot (the kernel's accumulate flag). fp32 whatever the convolution precision."""
import torch
from torch.autograd import Function

from ._lib import MbstdMember, MAX_GROUPS
from ._ops import lib, check, _c, _p, _stream
from .functional_multi import _fork_some

MAX_GROUP, MAX_HEADS = 16, 2


def check_group(G):
    """The group size of an enabled head: an int in 2..16."""
    if isinstance(G, bool) or not isinstance(G, int) or not 2 <= G <= MAX_GROUP:
        raise ValueError('mbstd (minibatch standard deviation) takes a group size in 2..%d (0: off), got %r' % (MAX_GROUP, G))
    return G


def _segs(fs, segs):
    segs = [f.shape[0] for f in fs] if segs is None else [int(s) for s in segs]
    if len(segs) != len(fs) or any(s < 1 or f.shape[0] % s for f, s in zip(fs, segs)):
        raise ValueError('minibatch standard deviation: one segment length per member that divides its rows, got %s for %s'
                         % (segs, [f.shape[0] for f in fs]))
    return tuple(segs)


def _check(w, fs, G, *per_head):
    n, H = len(fs), w.numel()
    check_group(G)
    if not 1 <= n <= MAX_GROUPS:
        raise ValueError('minibatch standard deviation takes 1..%d members per launch, got %d' % (MAX_GROUPS, n))
    if w.dim() != 1 or not 1 <= H <= MAX_HEADS:
        raise ValueError('minibatch standard deviation: w is [1] or [2], got %s' % (tuple(w.shape),))
    K = fs[0].shape[1] if fs[0].dim() == 2 else -1
    if any(f.dim() != 2 or f.shape[1] != K or f.shape[0] < 1 for f in fs):
        raise ValueError('minibatch standard deviation: members are [b, K] with one K, got %s' % ([tuple(f.shape) for f in fs],))
    for heads in per_head:
        if len(heads) != H or any(ts is not None and len(ts) != n for ts in heads):
            raise ValueError('minibatch standard deviation: one list per head (or None), one tensor per member')
        for ts in heads:
            for t, f in zip(ts or (), fs):
                if t is not None and t.numel() != f.shape[0]:
                    raise ValueError('minibatch standard deviation: a logit per row, got %s for %d rows' % (tuple(t.shape), f.shape[0]))
    return n, H, K


def _table(fs, segs, g=None, base=None, gam=None, y=None, stat=None, out=None):
    """g, base, y: per head a list of per-member tensors (or None); gam, stat, out: per-member tensors."""
    arr = (MbstdMember * len(fs))()
    for i, a in enumerate(arr):
        a.f, a.b, a.seg = fs[i].data_ptr(), fs[i].shape[0], segs[i]
        for key, heads in (('g', g), ('base', base), ('y', y)):
            for h, ts in enumerate(heads or ()):
                getattr(a, key)[h] = ts[i].data_ptr() if ts is not None and ts[i] is not None else None
        for key, ts in (('gam', gam), ('stat', stat), ('out', out)):
            setattr(a, key, ts[i].data_ptr() if ts is not None and ts[i] is not None else None)
    return arr


def _cc(heads):
    return [None if ts is None else [None if t is None else _c(t) for t in ts] for ts in heads]


def mbstd_fwd_raw(w, fs, bases, G, segs=None):
    """(ys, stats): ys[h] = [base_h + w_h·s] as [b, 1] tensors for every head with a `bases[h]` list (None: head not computed),
    stats = [s per row, [b]]; one launch."""
    w, fs, bases = _c(w), [_c(f) for f in fs], _cc(bases)
    n, H, K = _check(w, fs, G, bases)
    segs = _segs(fs, segs)
    new = lambda f, *shape: torch.empty((f.shape[0],) + shape, device=f.device, dtype=torch.float32)
    ys = [None if ts is None else [new(f, 1) for f in fs] for ts in bases]
    stats = [new(f) for f in fs]
    arr = _table(fs, segs, base=bases, y=ys, stat=stats)
    check(lib().t2v_mbstd_fwd(arr, n, _p(w), H, K, G, _stream()), 't2v_mbstd_fwd')
    return ys, stats


def mbstd_feat_raw(w, gs, fs, G, segs=None):
    """[a_q (f − μ)/(n K σ)] as [b, K] tensors, one launch. gs[h]: per-member dL/dy_h (entries, or the whole head, may be None)."""
    w, fs, gs = _c(w), [_c(f) for f in fs], _cc(gs)
    n, H, K = _check(w, fs, G, gs)
    segs = _segs(fs, segs)
    outs = [torch.empty_like(f) for f in fs]
    arr = _table(fs, segs, g=gs, out=outs)
    check(lib().t2v_mbstd_feat(arr, n, _p(w), H, K, G, _stream()), 't2v_mbstd_feat')
    return outs


def mbstd_second_raw(w, gs, fs, gams, G, segs=None, want_out=True, want_y=None):
    """(outs, ts, ys) of the feature adjoint's own adjoints for Γ = `gams`, one launch: outs = dL/df [b, K] (None without
    `want_out`), ts = t per row [b], ys[h] = [w_h·t] as the shape of a logit for the heads named in `want_y`."""
    w, fs, gs, gams = _c(w), [_c(f) for f in fs], _cc(gs), [_c(t) for t in gams]
    n, H, K = _check(w, fs, G, gs)
    segs = _segs(fs, segs)
    if len(gams) != n or any(t.shape != f.shape for t, f in zip(gams, fs)):
        raise ValueError('minibatch standard deviation: Γ has the shape of the features')
    outs = [torch.empty_like(f) for f in fs] if want_out else None
    ts = [torch.empty((f.shape[0],), device=f.device, dtype=torch.float32) for f in fs]
    ys = [[torch.empty((f.shape[0], 1), device=f.device, dtype=torch.float32) for f in fs] if h in (want_y or ()) else None
          for h in range(H)]
    arr = _table(fs, segs, g=gs, gam=gams, y=ys, stat=ts, out=outs)
    check(lib().t2v_mbstd_second(arr, n, _p(w), H, K, G, _stream()), 't2v_mbstd_second')
    return outs, ts, ys


def mbstd_weight_raw(gs, stats, H, K, G, out=None, accum=False):
    """Σ_members Σ_b g_h[b]·stat[b] as one [H] tensor (written into, or added onto, `out` when given), one launch."""
    gs, stats = _cc(gs), [_c(t) for t in stats]
    n = len(stats)
    if not 1 <= n <= MAX_GROUPS or len(gs) != H or any(ts is not None and len(ts) != n for ts in gs):
        raise ValueError('minibatch standard deviation: one gradient list per head, one statistic per member, 1..%d members' % MAX_GROUPS)
    if out is None:
        out = torch.empty((H,), device=stats[0].device, dtype=torch.float32)
    elif tuple(out.shape) != (H,) or not out.is_contiguous():
        raise ValueError('minibatch standard deviation: the weight gradient goes into a dense [%d] tensor' % H)
    arr = (MbstdMember * n)()
    for i, a in enumerate(arr):
        a.stat, a.b, a.seg = stats[i].data_ptr(), stats[i].shape[0], stats[i].shape[0]
        for h, ts in enumerate(gs):
            a.g[h] = ts[i].data_ptr() if ts is not None and ts[i] is not None else None
    check(lib().t2v_mbstd_weight(arr, n, _p(out), H, K, G, 1 if accum else 0, _stream()), 't2v_mbstd_weight')
    return out


def _aliases(ts, k):
    """k autograd aliases of every tensor of `ts` for k consumers inside a RECORDED backward (grouped forks); the tensors
    themselves when nothing is recorded or k < 2."""
    ts = list(ts)
    out = []
    for _ in range(k - 1):
        a, ts = _fork_some(ts)
        out.append(a)
    out.append(ts)
    return out


def _want_weight(ctx, idx):
    from . import functional as TF
    return ctx.needs_input_grad[idx] and TF._param_grads_enabled


def _weight_grad(w, cfg, gs, stats, K):
    """dL/dw over the given members: into w's gradient-sink slot when one is armed (None once it accumulated), else a Function.
    gs: heads-major flat list (len(heads)·n, entries may be None)."""
    from . import functional as TF
    G, n, _, heads = cfg
    H = w.numel()
    per = [None] * H
    for hi, h in enumerate(heads):
        per[h] = list(gs[hi * n:(hi + 1) * n])
    done, gw = TF._to_sink(w, lambda out, acc: mbstd_weight_raw(per, stats, H, K, G, out=out, accum=acc))
    if not done:
        gw = MbstdWeightG.apply((G, n, H, K, heads), *(list(gs) + list(stats)))
    return gw


def _sub(cfg, idx):
    G, n, segs, heads = cfg
    return (G, len(idx), tuple(segs[i] for i in idx), heads)


def _pick(ts, n, nh, idx):
    """The members `idx` of a heads-major flat list."""
    return [ts[hi * n + i] for hi in range(nh) for i in idx]


def _per_head(flat, n, heads, H):
    per = [None] * H
    for hi, h in enumerate(heads):
        per[h] = list(flat[hi * n:(hi + 1) * n])
    return per


class MbstdFwdG(Function):
    """ys = bases + w_h·s   —   args: (G, n, segs, heads), w, f_0.., then per head of `heads` base_0..; returns per head y_0.."""

    @staticmethod
    def forward(ctx, cfg, w, *ts):
        G, n, segs, heads = cfg
        fs, H = ts[:n], w.numel()
        ys, stats = mbstd_fwd_raw(w, fs, _per_head(ts[n:], n, heads, H), G, segs)
        ctx.save_for_backward(w, *fs)
        ctx.stats = stats                                      # (an intermediate of this Function alone: never an output)
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        return tuple(y for h in heads for y in ys[h])

    @staticmethod
    def backward(ctx, *gys):
        G, n, segs, heads = ctx.cfg
        nh = len(heads)
        w, fs = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        none = (None,) * n
        live = [i for i in range(n) if any(gys[hi * n + i] is not None for hi in range(nh))]
        if not live:
            return (None, None) + none + none * nh
        need = ctx.needs_input_grad
        lf = [i for i in live if need[2 + i]]
        lb = [j for j in range(nh * n) if gys[j] is not None and need[2 + n + j]]
        want_w = _want_weight(ctx, 1)
        k = sum(1 for u in (lb, lf, want_w) if u)
        al = iter(_aliases(gys, k) if k > 1 else [list(gys)] * k)
        d_b, d_f, d_w = [None] * (nh * n), list(none), None
        if lb:
            g = next(al)
            for j in lb:
                d_b[j] = g[j]
        if lf:
            g = next(al)
            res = MbstdFeatG.apply(_sub(ctx.cfg, lf), w, *(_pick(g, n, nh, lf) + [fs[i] for i in lf]))
            for i, r in zip(lf, res):
                d_f[i] = r
        if want_w:
            g = next(al)
            d_w = _weight_grad(w, _sub(ctx.cfg, live), _pick(g, n, nh, live), [ctx.stats[i] for i in live], fs[0].shape[1])
        return (None, d_w) + tuple(d_f) + tuple(d_b)


class MbstdFeatG(Function):
    """Fs[i] = a_q (f − μ)/(n K σ)   —   args: (G, n, segs, heads), w, per head g_0.. (entries may be None), f_0.."""

    @staticmethod
    def forward(ctx, cfg, w, *ts):
        G, n, segs, heads = cfg
        nh = len(heads)
        gs, fs = ts[:nh * n], ts[nh * n:]
        ctx.save_for_backward(w, *ts)
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        return tuple(mbstd_feat_raw(w, _per_head(gs, n, heads, w.numel()), fs, G, segs))

    @staticmethod
    def backward(ctx, *gams):
        G, n, segs, heads = ctx.cfg
        nh = len(heads)
        saved = ctx.saved_tensors
        w, gs, fs = saved[0], saved[1:1 + nh * n], saved[1 + nh * n:]
        none = (None,) * n
        live = [i for i in range(n) if gams[i] is not None]
        if not live:
            return (None, None) + none * nh + none
        need = ctx.needs_input_grad
        want_f = any(need[2 + nh * n + i] for i in live)
        want_y = tuple(hi for hi in range(nh) if any(gs[hi * n + i] is not None and need[2 + hi * n + i] for i in live))
        want_w = _want_weight(ctx, 1)
        d_g, d_f, d_w = [None] * (nh * n), list(none), None
        if not (want_f or want_y or want_w):
            return (None, None) + tuple(d_g) + tuple(d_f)
        m = len(live)
        res = MbstdSecondG.apply(_sub(ctx.cfg, live), want_f, want_y, w,
                                 *(_pick(gs, n, nh, live) + [fs[i] for i in live] + [gams[i] for i in live]))
        outs, ts, ys = res[:m], res[m:2 * m], res[2 * m:]
        for k, i in enumerate(live):
            if want_f and need[2 + nh * n + i]:
                d_f[i] = outs[k]
            for a, hi in enumerate(want_y):
                if gs[hi * n + i] is not None and need[2 + hi * n + i]:
                    d_g[hi * n + i] = ys[a * m + k].view_as(gs[hi * n + i])
        if want_w:
            d_w = _weight_grad(w, _sub(ctx.cfg, live), _pick(gs, n, nh, live), list(ts), fs[0].shape[1])
        return (None, d_w) + tuple(d_g) + tuple(d_f)


def _no_backward(name, grads):
    if any(g is not None for g in grads):
        raise RuntimeError('%s has no backward: the minibatch standard deviation head is differentiable twice (the gradient '
                           "penalty's sweep and its second backward), not three times" % name)


class MbstdSecondG(Function):
    """(dL/df_0.., t_0.., then per head of `want_y` w_h·t_0..) for Γ = dL/dF   —   args: (G, n, segs, heads), want_out, want_y, w,
    per head g_0.., f_0.., Γ_0..  (dL/df entries are None without `want_out`). Its backward is not written: it raises."""

    @staticmethod
    def forward(ctx, cfg, want_out, want_y, w, *ts):
        G, n, segs, heads = cfg
        nh = len(heads)
        gs, fs, gams = ts[:nh * n], ts[nh * n:nh * n + n], ts[nh * n + n:]
        outs, stats, ys = mbstd_second_raw(w, _per_head(gs, n, heads, w.numel()), fs, gams, G, segs, want_out=want_out,
                                           want_y=tuple(heads[hi] for hi in want_y))
        ctx.n_in = 4 + len(ts)
        ctx.set_materialize_grads(False)
        return tuple(outs if want_out else [None] * n) + tuple(stats) + tuple(y for hi in want_y for y in ys[heads[hi]])

    @staticmethod
    def backward(ctx, *grads):
        _no_backward('MbstdSecondG', grads)
        return (None,) * ctx.n_in


class MbstdWeightG(Function):
    """W [H] = Σ_i Σ_b g_h[b]·stat[b]   —   args: (G, n, H, K, heads), per head g_0.. (entries may be None), stat_0..
    Its backward is not written: it raises."""

    @staticmethod
    def forward(ctx, cfg, *ts):
        G, n, H, K, heads = cfg
        ctx.n_in = 1 + len(ts)
        ctx.set_materialize_grads(False)
        return mbstd_weight_raw(_per_head(ts[:len(heads) * n], n, heads, H), ts[len(heads) * n:], H, K, G)

    @staticmethod
    def backward(ctx, *grads):
        _no_backward('MbstdWeightG', grads)
        return (None,) * ctx.n_in


def mbstd_group(w, G, feats, bases, segs=None):
    """The minibatch-standard-deviation term on the logits of up to MAX_GROUPS members that share w, in ONE launch.
    bases[h] (h < w.numel()): the [b, 1] logits of head h per member, or None for a head that is not computed here; returns the
    same structure with w_h·s added. segs: a segment length per member (default: its row count)."""
    feats = list(feats)
    H = w.numel()
    bases = [None if ts is None else list(ts) for ts in bases]
    _check(w, feats, G, bases)
    heads = tuple(h for h in range(H) if bases[h] is not None)
    if not heads:
        raise ValueError('minibatch standard deviation: no head to add the term to')
    n = len(feats)
    res = MbstdFwdG.apply((G, n, _segs(feats, segs), heads), w, *(feats + [t for h in heads for t in bases[h]]))
    out = [None] * H
    for hi, h in enumerate(heads):
        out[h] = list(res[hi * n:(hi + 1) * n])
    return out
