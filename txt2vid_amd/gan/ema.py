"""Exponential moving average of the generator's weights (opt-in: `--G_ema DECAY`; the reference has none). DESIGN §16.

    e <- d e + (1 - d) p      after every generator update, d = DECAY once more than `start` updates were made, else 0

The update is one tick + one multi-tensor launch per 64 tensors (`t2v_ema_tick`, `t2v_ema_multi`), capturable, so it sits inside
the replayed HIP graph right behind the generator's optimiser step. Sampling and checkpoints read the average; `swapped()`
exchanges average and weights IN PLACE (same addresses) and refreshes the packed weight copies, so that inside the context every
kernel runs the averaged generator."""
import contextlib
from collections import OrderedDict

import torch

from .. import functional as TF
from .._lib import EmaJob

_PER_CALL = 64          # tensors per t2v_ema_multi call (= per launch)


def _like(p):
    """A tensor of its own laid out like `p` (same strides, tap-major ones included), holding a copy."""
    return torch.empty_strided(p.shape, p.stride(), dtype=p.dtype, device=p.device).copy_(p.detach())


def _jobs(pairs):
    arr = (EmaJob * len(pairs))()
    for a, (e, p) in zip(arr, pairs):
        a.e, a.p, a.n = e.data_ptr(), p.data_ptr(), e.numel()
    return arr


class GenAverage(object):
    """Moving average of the PARAMETERS of `gen`: one fp32 tensor per parameter, laid out like it, initialised as a copy.

    BatchNorm buffers are NOT averaged: `running_mean` / `running_var` already are moving averages, and the averaged generator
    uses the live ones (`num_batches_tracked` likewise).

    A tap-major parameter with structurally dead taps (`_t2v_live_taps`: the ConvLSTM weights on a 1x1 state) contributes only
    its live taps' contiguous rows to the update, as `optim.Adam.step` does: dead taps never change, so their average equals
    the initial copy for ever. `swapped()` exchanges whole tensors (it is off the hot path)."""

    def __init__(self, gen, decay, start=0):
        decay, start = float(decay), int(start)
        if not 0.0 <= decay < 1.0:
            raise ValueError('EMA decay must lie in [0, 1) (got %r)' % decay)
        if start < 0:
            raise ValueError('EMA start must be >= 0 (got %d)' % start)
        self.gen, self.decay, self.start = gen, decay, start
        self.names, self.params, self.avg = [], [], []
        for name, p in gen.named_parameters():
            if p.dtype != torch.float32:
                raise TypeError('the averaging kernels are fp32; parameter %s is %s' % (name, p.dtype))
            if not (p.is_contiguous() or TF.is_tap_major(p)):          # (is_tap_major raises on any other layout)
                raise ValueError('parameter layout not supported: %s has strides %s' % (name, p.stride()))
            self.names.append(name)
            self.params.append(p)
            self.avg.append(_like(p))
        if not self.params:
            raise ValueError('the generator has no parameters to average')
        self._repack_order = self.params[::-1]
        self.count = torch.zeros(1, dtype=torch.float32, device=self.params[0].device)      # generator updates seen (on the device)
        self._sig = self._update_calls = self._swap_calls = None

    # ---- job lists (device pointers: built on first use, again should a parameter have moved) -------------------------------
    def _build(self):
        sig = tuple(p.data_ptr() for p in self.params)
        if self._sig == sig:
            return
        for name, p, e in zip(self.names, self.params, self.avg):
            if not p.is_cuda:
                raise RuntimeError('the averaging kernels need device tensors: the HIP path has no CPU fallback')
            if e.device != p.device or e.stride() != p.stride() or e.shape != p.shape:
                raise ValueError('the average of %s no longer matches its parameter (moved or resized after construction)' % name)
        if self.count.device != self.params[0].device:
            raise ValueError('the update count lives on %s, the generator on %s' % (self.count.device, self.params[0].device))
        live, whole = [], []
        for p, e in zip(self.params, self.avg):
            whole.append((e, p))
            taps = getattr(p, '_t2v_live_taps', None)
            if taps is not None and not p.is_contiguous() and TF.is_tap_major(p):
                er, pr = TF.tap_rows(e), TF.tap_rows(p)
                live.extend((er[t], pr[t]) for t in taps)
            else:
                live.append((e, p))
        # (the views above only supply addresses; the ctypes arrays hold plain pointers into storages self.avg / gen keep alive)
        def calls(pairs):
            return [(_jobs(pairs[i:i + _PER_CALL]), len(pairs[i:i + _PER_CALL])) for i in range(0, len(pairs), _PER_CALL)]
        self._update_calls, self._swap_calls = calls(live), calls(whole)
        self.n_jobs = len(live)
        self.live_elements = sum(int(e.numel()) for e, _ in live)
        self._sig = sig

    # ---- hot path ----------------------------------------------------------------------------------------------------------
    def update(self):
        """One generator update happened: advance the count, fold the weights into the average. Capturable (no host read, no
        allocation): 1 + ceil(jobs / 64) launches on the current stream."""
        self._build()
        l, st = TF.lib(), TF._stream()
        TF.check(l.t2v_ema_tick(TF._p(self.count), st), 't2v_ema_tick')
        for arr, n in self._update_calls:
            TF.check(l.t2v_ema_multi(arr, n, self.decay, float(self.start), TF._p(self.count), 0.0, st), 't2v_ema_multi')

    # ---- sampling ----------------------------------------------------------------------------------------------------------
    def _swap(self):
        l, st = TF.lib(), TF._stream()
        for arr, n in self._swap_calls:
            TF.check(l.t2v_swap_multi(arr, n, st), 't2v_swap_multi')
        TF.bump_weight_epoch(self.params)       # the packed copies are stale ...
        # ... refresh them in place (same addresses: a captured graph keeps working). `repack_params` keeps one device job table
        # per parameter tuple and rebuilds it when a new packed variant appeared; a captured iteration has the optimiser's table
        # baked in, so this call walks the parameters in another order and thereby owns a table of its own
        TF.repack_params(self._repack_order)

    @contextlib.contextmanager
    def swapped(self):
        """Inside the context the generator IS the averaged generator for every kernel (and the average holds the live weights);
        on exit — also when the body raises — everything is exchanged back bit for bit."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('GenAverage.swapped() cannot run during stream capture')
        self._build()
        self._swap()
        try:
            yield self.gen
        finally:
            self._swap()

    # ---- checkpoints (host-only code: works on CPU tensors) ----------------------------------------------------------------
    @property
    def updates(self):
        """Generator updates seen so far (reads the device-resident count: a host sync)."""
        return int(round(float(self.count[0].item())))

    def state_dict(self):
        """{parameter name: averaged tensor} — the generator's parameter names, no buffers. The update count is `updates`."""
        return OrderedDict((k, e.detach()) for k, e in zip(self.names, self.avg))

    @torch.no_grad()
    def load_state_dict(self, state_dict=None, updates=0):
        """Missing keys (or no dict at all: a checkpoint written without an average) fall back to a copy of the live parameter."""
        state_dict = state_dict or {}
        unknown = sorted(set(state_dict) - set(self.names))
        if unknown:
            raise KeyError('averaged-generator state has keys the generator lacks: %s' % ', '.join(unknown[:5]))
        for k, p, e in zip(self.names, self.params, self.avg):
            src = state_dict.get(k)
            if src is None:
                src = p.detach()
            elif tuple(src.shape) != tuple(e.shape):
                raise ValueError('averaged %s has shape %s in the checkpoint, %s in the generator' % (k, tuple(src.shape), tuple(e.shape)))
            e.copy_(src)                        # keeps e's own layout whatever strides the file's tensor has
        self.count.fill_(float(int(updates)))
