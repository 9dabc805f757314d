"""Autograd surface of the frame-seed generator kernels (csrc/temporal.hip; txt2vid/models/tgan/temporal_gen.py:10-34).

One Function per transposed-convolution layer. A layer takes the RAW output of the layer in front together with that
layer's BatchNorm statistics `st` and applies BatchNorm + ReLU while it loads its operand, so each BatchNorm lives in two
Functions: its statistics come out of the producer's forward launch, its adjoint is finished by the consumer's backward
launch (which owns whole channels over the batch). Forward and backward are one launch each: 5 + 5 for the generator.
`st` ([mean | 1/std | scale | shift] per channel) carries no gradient: the BatchNorm adjoint inside the consumer's
backward already accounts for the dependence of the statistics on the batch.

Weight / bias / BatchNorm-affine gradients go into the gradient sink's arena slots like every other layer's. First-order
only: the generator never sits inside the gradient penalty's double backward. fp32 only.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import functional as TF
from ._ops import _stream, _p, _c, lib, check

TANH, ACC_W, ACC_B, ACC_GAMMA, ACC_BETA = 1, 2, 4, 8, 16


def _ss_ptr(st, C):
    """(scale, shift) half of a layer's statistics."""
    import ctypes
    return ctypes.c_void_p(st.data_ptr() + 2 * C * st.element_size()) if st is not None else ctypes.c_void_p(0)


def _grad_slot(p):
    """(buffer the kernel writes, accumulate?, what autograd receives) for the gradient of parameter `p`: its gradient-sink
    slot when the sink is armed (a fresh view the first time, None when accumulated — `functional._to_sink`), else a new
    tensor."""
    sink = TF._grad_sink
    if sink is not None and not torch.is_grad_enabled():
        base = p._base if p._base is not None else p
        slot = sink.take(base)
        if slot is not None:
            flat, acc = slot
            v = flat.view(p.shape)
            return v, acc, (None if acc else v)
    t = torch.empty_like(p)
    return t, False, t


def _backward(g, z, w, x, st_in, need_x, params):
    """One `t2v_tseed_bwd` launch: dL/dx (through the BatchNorm in front when st_in is given) and the gradients of
    params = (weight, bias, gamma_in, beta_in) (the last two None without a BatchNorm in front)."""
    B, Cin, Lin = x.shape
    _, Cout, K = w.shape
    gin = torch.empty_like(x) if (need_x or st_in is not None) else None     # (dgamma / dbeta come with dL/dx)
    slots = [(_grad_slot(p) if p is not None else (None, False, None)) for p in params]
    flags = TANH if z is not None else 0
    for (_, acc, _), bit in zip(slots, (ACC_W, ACC_B, ACC_GAMMA, ACC_BETA)):
        flags |= bit if acc else 0
    (dw, _, rw), (db, _, rb), (dg, _, rg), (dbt, _, rbt) = slots
    check(lib().t2v_tseed_bwd(_p(g), _p(z), _p(w), _p(x), _p(st_in), _p(gin), _p(dw), _p(db), _p(dg), _p(dbt), B, Cin, Cout, Lin, K,
                              flags, _stream()), 't2v_tseed_bwd')
    return (gin if need_x else None), rw, rb, rg, rbt


class TSeedBN(Function):
    """dc_l of the frame-seed generator on relu(bn_{l-1}(x)) (x as is for dc0): returns (y, st) — y [B, Cout, Lout] before
    bn_l, st its statistics (training) or the running-buffer scale / shift (eval). Running buffers and the step counter are
    updated by the same launch."""

    @staticmethod
    def forward(ctx, x, st_in, w, b, gamma_in, beta_in, gamma, beta, rmean, rvar, counter, training, momentum, eps):
        x = _c(x)
        B, Cin, Lin = x.shape
        _, Cout, K = w.shape
        if w.shape[0] != Cin or (st_in is not None and st_in.numel() != 4 * Cin) or gamma.numel() != Cout:
            raise ValueError('frame-seed layer: input [%d, %d, %d] does not fit weight %s' % (B, Cin, Lin, tuple(w.shape)))
        Lout = 2 * Lin if K == 4 else Lin
        y = torch.empty((B, Cout, Lout), device=x.device, dtype=torch.float32)
        st = torch.empty((4 * Cout,), device=x.device, dtype=torch.float32)
        check(lib().t2v_tseed_fwd_bn(_p(x), _ss_ptr(st_in, Cin), _p(w), _p(b), _p(gamma), _p(beta), _p(y), _p(st), _p(rmean), _p(rvar),
                                     _p(counter if training else None), B, Cin, Cout, Lin, K, momentum, eps, int(training), _stream()),
              't2v_tseed_fwd_bn')
        ctx.mark_non_differentiable(st)
        if training:
            ctx.save_for_backward(x, st_in, w, b, gamma_in, beta_in)
        ctx.training = training
        return y, st

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, gst):
        if not ctx.training:
            raise RuntimeError('the frame-seed generator has no eval-mode backward')
        x, st_in, w, b, gamma_in, beta_in = ctx.saved_tensors
        gx, gw, gb, gg, gbt = _backward(_c(gy), None, w, x, st_in, ctx.needs_input_grad[0], (w, b, gamma_in, beta_in))
        return gx, None, gw, gb, gg, gbt, None, None, None, None, None, None, None, None


class TSeedTanh(Function):
    """dc4 + tanh on relu(bn3(x)): z [B, Cout, 16] — contiguous, so it already is the merged-frames [B*16, C, h, w] tensor of
    the reference's `view(B, 16, -1, h, w)` + `merge_frames`."""

    @staticmethod
    def forward(ctx, x, st_in, w, b, gamma_in, beta_in):
        x = _c(x)
        B, Cin, Lin = x.shape
        _, Cout, K = w.shape
        if K != 4 or Lin != 8 or w.shape[0] != Cin or st_in.numel() != 4 * Cin:
            raise ValueError('the tanh layer of the frame-seed generator is dc4: k = 4 on 8 positions')
        z = torch.empty((B, Cout, 2 * Lin), device=x.device, dtype=torch.float32)
        check(lib().t2v_tseed_fwd_tanh(_p(x), _ss_ptr(st_in, Cin), _p(w), _p(b), _p(z), B, Cin, Cout, Lin, _stream()), 't2v_tseed_fwd_tanh')
        ctx.save_for_backward(x, st_in, w, b, gamma_in, beta_in, z)
        return z

    @staticmethod
    @once_differentiable
    def backward(ctx, gz):
        x, st_in, w, b, gamma_in, beta_in, z = ctx.saved_tensors
        gx, gw, gb, gg, gbt = _backward(_c(gz), z, w, x, st_in, ctx.needs_input_grad[0], (w, b, gamma_in, beta_in))
        return gx, None, gw, gb, gg, gbt


def tseed_bn(x, st_in, dc, bn_in, bn, training):
    """One BatchNorm-producing layer: dc = the ConvTranspose1d, bn_in = the BatchNorm1d whose statistics st_in are (None for
    dc0), bn = the BatchNorm1d behind dc. Returns (raw output, st)."""
    if bn.momentum is None or not bn.affine or not bn.track_running_stats:
        raise NotImplementedError('only the default BatchNorm1d configuration is built')
    return TSeedBN.apply(x, st_in, dc.weight, dc.bias, None if bn_in is None else bn_in.weight, None if bn_in is None else bn_in.bias,
                         bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bool(training), float(bn.momentum),
                         float(bn.eps))


def tseed_tanh(x, st_in, dc, bn_in):
    return TSeedTanh.apply(x, st_in, dc.weight, dc.bias, bn_in.weight, bn_in.bias)
