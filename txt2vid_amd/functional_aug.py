"""Differentiable augmentation of the discriminator's inputs (DiffAugment, Zhao et al. 2020; opt-in through `--D_aug`, not in the
reference): the shared definition of the transformation and the autograd surface of its two grouped kernels
(csrc/diffaug.hip `t2v_diffaug_fwd` / `t2v_diffaug_bwd`). DESIGN §17.

THE DEFINITION (kernels, `aug_params` and the tests' restatement all follow it). The policy is a subset of
color, translation, cutout, applied in that order, one transformation per clip [C, T, S, S], constant over its frames. A call
consumes one block u [B, K] of uniforms in [0, 1), K = 8, one row per base sample:

    column 0  brightness   x + b,              b = u0 - 0.5
    column 1  saturation   (x - m) s + m,      s = 2 u1,     m = the voxel's mean over channels   (identity for C = 1)
    column 2  contrast     (x - mu) c + mu,    c = u2 + 0.5, mu = the mean of the whole clip after brightness and saturation
                                                              = mean(input clip) + b  (saturation keeps the channel mean)
    column 3  tx = min(floor(u3 (2r + 1)), 2r) - r,  r = floor(S / 8 + 0.5)
    column 4  ty, the same from u4;            out(h, w) = in(h - ty, w - tx), 0 outside the frame
    column 5  cx = min(floor(u5 n), n - 1),    size = floor(S / 2 + 0.5), n = S + 1 - size % 2
    column 6  cy, the same from u6;            out = 0 for columns in [cx - size // 2, cx - size // 2 + size) and rows in the same
                                               range around cy
    column 7  unused (it pads a row to 32 bytes)

The products u3 (2r + 1), u5 n, ... are taken EXACTLY (an fp32 value times a small integer; float64 holds it), so the integer
parameters are the same on every side. Pyramid level l re-derives the integers from the same row for its own S; under
--subsample_input sample j of level l reads the row of base sample j * 2^l, the sample it was sub-sampled from, so a clip gets
the same transformation at every scale.

The map is affine per clip. Adjoint: mask and shift the incoming gradient back, then contrast c g + (1 - c) mean_clip(g), then
saturation s g + (1 - s) mean_channels(g); brightness is the identity. The backward is ONCE differentiable: the gradient
penalty's interpolates are formed from the already augmented clips and stay leaves, so no second-order adjoint is needed.
fp32 whatever the convolution precision.

ADAPTIVE STRENGTH (ADA, Karras et al. 2020; opt-in through `--D_aug_p` / `--D_ada`; kernels `t2v_diffaug_gated_fwd` /
`_bwd`, controller `t2v_ada_update` behind gan/ada.py). THE DEFINITION, stated once:

  Gating. Every parameter block u [B, 8] gets a GATE block g [B, 8] of uniforms in [0, 1), drawn immediately after u from the
  same generator. Columns 0, 1, 2 gate color, translation, cutout; columns 3-7 are unused. Clip j of a member reads gate row
  j * row_stride, the rule its parameter row follows, so a clip gets the same gates at every pyramid level. The effective policy
  of a clip is   policy & (1 [g0 < p] | 2 [g1 < p] | 4 [g2 < p])   with a strict fp32 < (g == p: not applied) and p read from
  DEVICE memory by the launch; the rest of the transformation is unchanged. So p = 1 is the ungated transformation bit for bit,
  p = 0 is a copy, a clip whose effective policy is 0 is copied in the forward and in the adjoint, and a clip without live color
  needs no clip sum. Wherever a parameter block is reused its gate block is reused with it.

  Statistic. r_t = mean over pyramid levels l and pairs j < b_l of sgn(u_r[l][j] - u_f[l][j]), sgn(0) = 0, over the
  unconditional real and generated logits that enter the `lu` term of the D loss of the FIRST discriminator (the paired form: the
  default loss, RSGAN, is relativistic and its logits have no anchored zero, so the paper's E[sign(D(real))] means nothing here).

  Controller. Device state ada float32[8] = {p, sum of sgn in the window, pairs in the window, D steps in the window, 0, 0, 0, 0}.
  Per D step, behind that step's D forward, ONE launch adds the step's sign sum and pair count and increments ada[3]; when
  ada[3] >= interval it sets p <- clamp(p + sgn(ada[1] / ada[2] - target) * step, 0, 1) and zeroes ada[1..3].
  step = B * interval / (1000 * kclips), computed on the host in double and passed as one fp32. The window sums are small
  integers (exact in fp32 in any order) and the update is one fp32 add and two clamps, so a numpy float32 restatement agrees
  with the device bitwise. Order within D step j: augment with the current p, D forward, observe / update; the next augmentation
  launch in stream order (the G step's too) sees the new p.

  THE p-INVARIANT. The backward re-reads the gates and p instead of keeping a snapshot. p is written by the observe launch
  alone, which sits behind the D forward: inside a D step the augmentation's forward and (if any) backward both precede it in
  stream order or carry no gradient at all (the D step's clips are detached), and a G step has no write between its forward and
  its backward. Forward and backward of one augmentation therefore see one value of p.

GEOMETRIC AUGMENTATION (ADA's x-flip, isotropic scaling and rotation; opt-in through the names flip, scale, rotate of `--D_aug`,
not in the reference; kernels csrc/geoaug.hip `t2v_geoaug_fwd` / `_bwd`). THE DEFINITION, stated once (the header
comment, `geo_params`, the tests' restatement and DESIGN follow it):

  Draws. A site whose policy has a geometric bit consumes one more block v [B, 8] of uniforms in [0, 1), drawn from the same
  generator directly behind that site's u (and g, when gated): u_real, [g_real], v_real, u_fake, [g_fake], v_fake. u is drawn even
  if the policy holds geometric names only. Clip j of a member reads row j * row_stride of v, the rule u follows, so a clip gets
  the same transformation at every pyramid level: scale and angle are resolution-free, coordinates relative to the frame centre.

    column 0  flip     f = -1 (mirror left <-> right) iff v0 < 0.5, else +1
    column 1  scale    s = exp2((2 v1 - 1) * 0.4)         (+-2 sigma of ADA's log-normal with sigma = 0.2 octaves; bounded, so
                                                           that the adjoint's search window is bounded)
    column 2  rotate   theta = (2 v2 - 1) * pi / 6
    columns 3-7        unused

  A transformation that is not in the policy or not live takes f = +1, s = 1, theta = 0. The three constants are this
  definition's and untuned for video.

  Gating. No new gate block: columns 3, 4, 5 of the gate block g that is already drawn gate flip, scale, rotate. The effective
  geometric policy of a clip is   policy & (8 [g3 < p] | 16 [g4 < p] | 32 [g5 < p])   with the same strict fp32 < and p read from
  device memory when the launch runs. THE p-INVARIANT carries over: the new launches sit where the old ones sit relative to
  `t2v_ada_update`; the controller, its statistic and its state are unchanged.

  Map. One bilinear resampling per clip [C, T, S, S], constant over its frames and channels, run BEFORE colour -> translation ->
  cutout (ADA's order: geometry first, cutout last). Output pixel (h, w) has the centre coordinates xo = w + 0.5 - S/2,
  yo = h + 0.5 - S/2 and samples the input at

      x_src = f ( cos(theta) xo + sin(theta) yo) / s
      y_src =   (-sin(theta) xo + cos(theta) yo) / s

  flip, then scale, then rotation, written directly as the sampling matrix (nobody inverts anything). Its four entries
  f cos / s, f sin / s, -sin / s, cos / s are formed in double from the fp32 draw and rounded ONCE to fp32; per-pixel
  coordinates and weights are fp32. Then px = x_src + S/2 - 0.5, x0 = floor(px), wx = px - x0 (the same for y), and the value is
  the bilinear blend of the four taps; a tap outside the frame contributes zero (this project's translation convention; ADA
  reflects). Two consequences: f = 1, s = 1, theta = 0 gives px = w exactly and the output equals the input; a pure flip gives
  px = S - 1 - w exactly, an exact mirror. (Through the blend -0.0 comes out as +0.0; a clip whose effective policy is 0 is a
  plain copy.)

  Adjoint. The map is linear per clip and the backward ONCE differentiable, as above. It is a deterministic gather without
  atomics: input pixel i receives from the output pixels whose source position lies within (-1, 1) of i in both axes; their
  pre-image is a parallelogram whose bounding box has half-width s (|cos| + |sin|) <= 1.32 * 1.37 < 1.81, so the 5 x 5 output
  pixels around the rounded pre-image of i hold them all. Each candidate's weight comes from the device function the forward
  uses, and the candidates are summed in row-major order: the backward is the exact transpose of the forward, weight by weight.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ._lib import AugMember, MAX_GROUPS
from ._ops import _stream, _c, lib, check

K = 8                                                     # uniforms per base sample (T2V_AUG_K)
COLOR, TRANSLATION, CUTOUT = 1, 2, 4                      # policy bits (T2V_AUG_*)
FLIP, SCALE, ROTATE = 8, 16, 32                           # the geometric ones: their own launch, in front (csrc/geoaug.hip)
GEO = FLIP | SCALE | ROTATE
NAMES = ('color', 'translation', 'cutout', 'flip', 'scale', 'rotate')
SCALE_OCTAVES = 0.4                                       # s = exp2((2 v1 - 1) * 0.4)
PI_6 = 0.5235987755982988                                 # theta = (2 v2 - 1) * pi / 6; the double the kernel uses


def parse_policy(text):
    """'color,cutout' -> policy bits ('' or None -> 0). ValueError on an unknown or empty name."""
    if not text:
        return 0
    bits = 0
    for name in str(text).split(','):
        name = name.strip()
        if name not in NAMES:
            raise ValueError('unknown augmentation %r (choose from %s)' % (name, ', '.join(NAMES)))
        bits |= 1 << NAMES.index(name)
    return bits


def _index(u, n):
    """min(floor(u n), n - 1) as int64, the product taken exactly in float64."""
    return torch.clamp(torch.floor(u.double() * n).long(), 0, n - 1)


def aug_params(u, S):
    """The parameters of one block u [B, K] (fp32) for frames of side S, per base sample: a dict of
    b, s, c (float64, exact functions of the fp32 draws), tx, ty (int64 in [-r, r]), x0, y0 (int64, first column / row of the cut
    box, may be negative) and size, r (ints)."""
    if u.dim() != 2 or u.shape[1] != K:
        raise ValueError('an augmentation block is [B, %d], got %s' % (K, tuple(u.shape)))
    S = int(S)
    r = (S + 4) // 8                                   # floor(S / 8 + 0.5)
    size = (S + 1) // 2                                # floor(S / 2 + 0.5)
    n = S + 1 - size % 2
    ud = u.double()
    return dict(b=ud[:, 0] - 0.5, s=2.0 * ud[:, 1], c=ud[:, 2] + 0.5,
                tx=_index(u[:, 3], 2 * r + 1) - r, ty=_index(u[:, 4], 2 * r + 1) - r,
                x0=_index(u[:, 5], n) - size // 2, y0=_index(u[:, 6], n) - size // 2, size=size, r=r)


def geo_params(v, policy=GEO):
    """The geometric parameters of one block v [B, K] (fp32), per base sample: a dict of f (+-1), s, theta (float64, exact
    functions of the fp32 draws up to the rounding of exp2) and M [B, 2, 2] (float32), the sampling matrix
    [[f cos / s, f sin / s], [-sin / s, cos / s]] formed in float64 and rounded once. `policy`: the geometric bits that are live,
    one int for the block or one per row; a transformation that is not live takes f = +1, s = 1, theta = 0."""
    if v.dim() != 2 or v.shape[1] != K:
        raise ValueError('an augmentation block is [B, %d], got %s' % (K, tuple(v.shape)))
    B = v.shape[0]
    bits = torch.as_tensor(policy, dtype=torch.int64).reshape(-1).expand(B) if not torch.is_tensor(policy) else policy.long().expand(B)
    vd = v.detach().cpu().double()
    one, zero = torch.ones(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    f = torch.where(((bits & FLIP) != 0) & (v.detach().cpu()[:, 0] < 0.5), -one, one)
    s = torch.where((bits & SCALE) != 0, torch.exp2((2.0 * vd[:, 1] - 1.0) * SCALE_OCTAVES), one)
    theta = torch.where((bits & ROTATE) != 0, (2.0 * vd[:, 2] - 1.0) * PI_6, zero)
    c, sn = torch.cos(theta), torch.sin(theta)
    M = torch.stack([torch.stack([(f * c) / s, (f * sn) / s], 1), torch.stack([(-sn) / s, c / s], 1)], 1).float()
    return dict(f=f, s=s, theta=theta, M=M)


def _members(srcs, dsts, us, strides, policy):
    arr = (AugMember * len(srcs))()
    for a, x, y, u, st in zip(arr, srcs, dsts, us, strides):
        N, Cc, T, H, W = x.shape
        a.x, a.y, a.u = x.data_ptr(), y.data_ptr(), u.data_ptr()
        a.N, a.C, a.T, a.S = N, Cc, T, H
        a.row_stride, a.rows, a.policy = int(st), int(u.shape[0]), policy
    return arr


def _gate_ptrs(gates):
    import ctypes
    return (ctypes.c_void_p * len(gates))(*[None if g is None else g.data_ptr() for g in gates])


def _prepare(us, strides, gate, xs):
    """The checks both augmentation launches share; returns the contiguous (xs, us, gate)."""
    if not 1 <= len(xs) <= MAX_GROUPS:
        raise ValueError('1 to %d tensors per augmentation launch, got %d' % (MAX_GROUPS, len(xs)))
    if len(us) != len(xs) or len(strides) != len(xs):
        raise ValueError('one parameter block and one row stride per tensor')
    xs = [_c(x) for x in xs]
    us = [_c(u) for u in us]
    for x, u in zip(xs, us):
        if x.dim() != 5 or x.shape[3] != x.shape[4]:
            raise ValueError('augmentation takes clips [N, C, T, S, S] with square frames, got %s' % (tuple(x.shape),))
        if u.dim() != 2 or u.shape[1] != K:
            raise ValueError('an augmentation block is [B, %d], got %s' % (K, tuple(u.shape)))
    if gate is not None:
        gates, p = gate
        if len(gates) != len(xs):
            raise ValueError('one gate block (or None) per tensor')
        gates = [None if g is None else _c(g) for g in gates]
        for g, u in zip(gates, us):
            if g is not None and g.shape != u.shape:
                raise ValueError('a gate block has the shape of its parameter block %s, got %s' % (tuple(u.shape), tuple(g.shape)))
        p = _c(p)
        if p.numel() < 1:
            raise ValueError('p is one float in device memory')
        gate = (gates, p)
    return xs, us, gate


class DiffAug(Function):
    """ys = T(xs): ONE forward launch for all members; ONE backward launch over the members that require a gradient (none: no
    launch). The parameter blocks carry no gradient (host draws). `gate`: None, or (gates, p) — one gate block (or None: that
    member is ungated) per tensor and the device float p; then both launches are the gated ones and the backward re-reads gates
    and p (p is not snapshotted: see THE p-INVARIANT in the module docstring)."""

    @staticmethod
    def forward(ctx, policy, us, strides, gate, *xs):
        xs, us, gate = _prepare(us, strides, gate, xs)
        ys = [torch.empty_like(x) for x in xs]
        if gate is None:
            check(lib().t2v_diffaug_fwd(_members(xs, ys, us, strides, policy), len(xs), _stream()), 't2v_diffaug_fwd')
        else:
            check(lib().t2v_diffaug_gated_fwd(_members(xs, ys, us, strides, policy), _gate_ptrs(gate[0]), len(xs), gate[1].data_ptr(),
                                              _stream()), 't2v_diffaug_gated_fwd')
        ctx.set_materialize_grads(False)
        ctx.cfg = (policy, tuple(strides))
        ctx.us = us                                    # (plain tensors that never require grad: no saved-tensor hooks needed)
        ctx.gate = gate
        ctx.mark_non_differentiable(*[y for y, need in zip(ys, ctx.needs_input_grad[4:]) if not need])
        return tuple(ys)

    @staticmethod
    @once_differentiable
    def backward(ctx, *gys):
        policy, strides = ctx.cfg
        live = [i for i, g in enumerate(gys) if g is not None and ctx.needs_input_grad[4 + i]]
        gxs = [None] * len(gys)
        if live:
            gs = [_c(gys[i]) for i in live]
            outs = [torch.empty_like(g) for g in gs]
            ms = _members(gs, outs, [ctx.us[i] for i in live], [strides[i] for i in live], policy)
            if ctx.gate is None:
                check(lib().t2v_diffaug_bwd(ms, len(live), _stream()), 't2v_diffaug_bwd')
            else:
                # the same gates and the SAME p the forward saw: nothing writes p between the two (THE p-INVARIANT)
                gates, p = ctx.gate
                check(lib().t2v_diffaug_gated_bwd(ms, _gate_ptrs([gates[i] for i in live]), len(live), p.data_ptr(), _stream()),
                      't2v_diffaug_gated_bwd')
            for i, o in zip(live, outs):
                gxs[i] = o
        return (None, None, None, None) + tuple(gxs)


def diffaug(xs, us, strides, policy, gates=None, p=None):
    """Augment the clips `xs` (a list of [N, C, T, S, S] device tensors) in one launch; member i reads row j * strides[i] of its
    block us[i] [B, K] for its clip j. `policy`: bits or a comma-separated string. Returns the list of augmented clips.
    `gates` (a list of gate blocks [B, K], None entries for ungated members) and `p` (a device float32 tensor, read when the
    launch runs) come together: each transformation is then applied per clip with probability p (see ADAPTIVE STRENGTH above)."""
    bits = parse_policy(policy) if isinstance(policy, str) else int(policy)
    bits &= ~GEO                                       # the geometric names are geoaug's, in front of this launch
    if not bits:
        return list(xs)
    if (gates is None) != (p is None):
        raise ValueError('gates and p come together')
    gate = None if gates is None else (tuple(gates), p)
    return list(DiffAug.apply(bits, tuple(us), tuple(strides), gate, *xs))


class GeoAug(Function):
    """ys = R(xs), the geometric resampling: ONE forward launch for all members; ONE backward launch over the members that require
    a gradient (none: no launch). `gate` as in DiffAug; the backward re-reads gates and p (THE p-INVARIANT)."""

    @staticmethod
    def forward(ctx, policy, vs, strides, gate, *xs):
        xs, vs, gate = _prepare(vs, strides, gate, xs)
        ys = [torch.empty_like(x) for x in xs]
        check(lib().t2v_geoaug_fwd(_members(xs, ys, vs, strides, policy), *_gate_args(gate, range(len(xs))), _stream()),
              't2v_geoaug_fwd')
        ctx.set_materialize_grads(False)
        ctx.cfg = (policy, tuple(strides))
        ctx.vs = vs
        ctx.gate = gate
        ctx.mark_non_differentiable(*[y for y, need in zip(ys, ctx.needs_input_grad[4:]) if not need])
        return tuple(ys)

    @staticmethod
    @once_differentiable
    def backward(ctx, *gys):
        policy, strides = ctx.cfg
        live = [i for i, g in enumerate(gys) if g is not None and ctx.needs_input_grad[4 + i]]
        gxs = [None] * len(gys)
        if live:
            gs = [_c(gys[i]) for i in live]
            outs = [torch.empty_like(g) for g in gs]
            ms = _members(gs, outs, [ctx.vs[i] for i in live], [strides[i] for i in live], policy)
            check(lib().t2v_geoaug_bwd(ms, *_gate_args(ctx.gate, live), _stream()), 't2v_geoaug_bwd')
            for i, o in zip(live, outs):
                gxs[i] = o
        return (None, None, None, None) + tuple(gxs)


def _gate_args(gate, which):
    """(gates, n, p) of a geoaug launch over the members `which`: NULL, n, NULL for the ungated form."""
    which = list(which)
    if gate is None:
        return None, len(which), None
    gates, p = gate
    return _gate_ptrs([gates[i] for i in which]), len(which), p.data_ptr()


def geoaug(xs, vs, strides, policy, gates=None, p=None):
    """Resample the clips `xs` (a list of [N, C, T, S, S] device tensors) in one launch with the geometric part (flip, scale,
    rotate) of `policy`; member i reads row j * strides[i] of its block vs[i] [B, K] for its clip j. The other bits of `policy`
    are diffaug's and ignored here; without a geometric bit the clips come back as they are, without a launch. `gates` and `p`
    as in diffaug: the gate blocks of the site (columns 3, 4, 5) and the device float read when the launch runs."""
    bits = (parse_policy(policy) if isinstance(policy, str) else int(policy)) & GEO
    if not bits:
        return list(xs)
    if (gates is None) != (p is None):
        raise ValueError('gates and p come together')
    gate = None if gates is None else (tuple(gates), p)
    return list(GeoAug.apply(bits, tuple(vs), tuple(strides), gate, *xs))
