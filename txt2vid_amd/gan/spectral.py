"""Spectral normalisation of the discriminator's weights (opt-in: `--D_sn`; Miyato et al. 2018; the reference has none).
DESIGN §18.

Every `Conv3d` / `Linear` weight W of the discriminators, seen as a matrix [M = Cout, K = Cin kD kH kW], is replaced by
What = W / sigma, sigma an estimate of W's largest singular value kept current by power iteration on persistent vectors
u [M], v [K] (the semantics of `torch.nn.utils.spectral_norm`, eps = 1e-12):

    refresh:  t = W^T u ; v = t / max(|t|, eps) ; s = W v ; u = s / max(|s|, eps) ; sigma = u . s ; What = W / sigma
    backward: c = <G, What> ; dL/dW = (G - c u v^T) / sigma          (G = dL/dWhat; u, v constants, as in torch)

torch refreshes on every training forward; here ONE refresh follows every discriminator optimiser step (plus `n_init` at
set-up), so all D and G forwards between two D updates multiply with the same What.

The registered Parameter `weight` holds What while the discriminator runs: the convolution path, the packed-weight caches, the
gradient sink and the arenas (all keyed on the Parameter's identity) stay as they are. The master W lives here, next to u, v
and sigma. The optimiser calls back through `Adam.weight_hook` / `SGD.weight_hook`:

    project_grads()   after the gradient flush, before the update: maps the gradients and puts W back into `weight`
    refresh()         after the update, before the weights are re-packed: saves W, power iteration, `weight` = What

Both are grouped launches over all layers (`t2v_sn_project`: 3 launches, `t2v_sn_refresh`: 5 n_power_iterations + 1, per 32
layers), capturable, so they sit inside the replayed HIP graph at fixed addresses."""
from collections import OrderedDict

import torch
import torch.nn as nn

from .. import functional as TF
from .._lib import SnJob, SN_MAX_JOBS, T2VError

STATE_SUFFIXES = ('_orig', '_u', '_v', '_sigma')


def normalised_layers(discrims):
    """[(state key, module)] of every layer whose weight is normalised: all Conv3d and Linear modules, in module order; the key is
    '<index of the discriminator>.<module path>.weight'."""
    out, seen = [], set()
    for i, d in enumerate(discrims):
        for name, m in d.named_modules():
            if isinstance(m, (nn.Conv3d, nn.Linear)) and id(m.weight) not in seen:
                seen.add(id(m.weight))
                out.append(('%d.%s.weight' % (i, name), m))
    return out


def initial_u(M, generator, eps=1e-12):
    """u ~ N(0, 1) on the host generator, normalised like torch's `F.normalize(u, dim=0, eps)`."""
    u = torch.randn(M, generator=generator, dtype=torch.float32)
    return u / max(float(u.norm()), eps)


class SpectralNorm(object):
    """Spectral normalisation of every Conv3d / Linear weight of `discrims` (biases, `Attention3d.gamma` and everything outside the
    discriminators are left alone).

    `state`: a dict written by `state_dict()` — the run continues with that W, u, v, sigma bit for bit and `weight` (already What in
    such a checkpoint) is not touched. Without it the current weights are taken as W, u is drawn from a host generator seeded with
    `seed` (the same on every data-parallel rank, like the weights) and `n_init` power iterations run before the first What."""

    def __init__(self, discrims, n_power_iterations=1, eps=1e-12, n_init=15, seed=0, state=None):
        self.n_iter, self.eps, self.n_init = int(n_power_iterations), float(eps), int(n_init)
        if self.n_iter < 1 or self.n_init < 1:
            raise ValueError('n_power_iterations and n_init must be >= 1 (got %d and %d)' % (self.n_iter, self.n_init))
        if not self.eps > 0:
            raise ValueError('eps must be positive (got %r)' % eps)
        layers = normalised_layers(discrims)
        if not layers:
            raise ValueError('the discriminators have no Conv3d / Linear weight to normalise')
        self.names, self.params = [k for k, _ in layers], [m.weight for _, m in layers]
        for k, p in zip(self.names, self.params):
            if p.dtype != torch.float32:
                raise TypeError('the spectral-norm kernels are fp32; %s is %s' % (k, p.dtype))
            if not p.is_contiguous():
                raise ValueError('the spectral-norm kernels need contiguous weights; %s has strides %s' % (k, p.stride()))
        for k, p in zip(self.names, self.params):
            if not p.is_cuda:
                raise RuntimeError('the spectral-norm kernels need device tensors (%s is on %s): the HIP path has no CPU fallback'
                                   % (k, p.device))
        self.shapes = [(int(p.shape[0]), int(p.numel() // p.shape[0])) for p in self.params]
        dev = self.params[0].device
        self.orig = [torch.empty_like(p) for p in self.params]
        self.u = [torch.empty(M, dtype=torch.float32, device=dev) for M, _ in self.shapes]
        self.v = [torch.zeros(K, dtype=torch.float32, device=dev) for _, K in self.shapes]
        self.sigma = [torch.zeros(1, dtype=torch.float32, device=dev) for _ in self.shapes]
        self._refresh_calls = self._project_calls = self._project_sig = None
        self._ws = None
        self.refreshes = 0                     # refresh() calls issued (a captured one counts once; host-side bookkeeping)
        self._alloc_workspace()
        if state is not None:
            self.load_state_dict(state)
        else:
            gen = torch.Generator().manual_seed(int(seed))
            with torch.no_grad():
                for p, w, u, (M, _) in zip(self.params, self.orig, self.u, self.shapes):
                    w.copy_(p.detach())
                    u.copy_(initial_u(M, gen, self.eps))
            self._launch_refresh(self.n_init, from_param=False)
            TF.bump_weight_epoch(self.params)
            TF.repack_params(self.params[::-1])        # (a table of its own: the optimiser's is baked into captured graphs)

    # ---- job tables (host arrays of device pointers; rebuilt when a gradient moved) ------------------------------------------
    def _jobs(self, idx, grads=None):
        arr = (SnJob * len(idx))()
        for a, i in zip(arr, idx):
            a.w, a.what, a.u, a.v = self.orig[i].data_ptr(), self.params[i].data_ptr(), self.u[i].data_ptr(), self.v[i].data_ptr()
            a.sigma, a.g = self.sigma[i].data_ptr(), (grads[i].data_ptr() if grads is not None else None)
            a.M, a.K = self.shapes[i]
        return arr

    def _calls(self, idx, grads=None):
        calls = []
        for at in range(0, len(idx), SN_MAX_JOBS):
            part = idx[at:at + SN_MAX_JOBS]
            arr = self._jobs(part, grads)
            need = int(TF.lib().t2v_sn_ws_floats(arr, len(part)))
            if need < 0:
                raise T2VError('t2v_sn_ws_floats failed with status %d' % need)
            calls.append((arr, len(part), need))
        assert max(c[2] for c in calls) <= self._ws.numel()
        return calls

    def _alloc_workspace(self):
        """ONE workspace for every call this object will ever make (they run back to back on one stream), allocated at
        construction: a call's need is the sum of its jobs' needs, so the SN_MAX_JOBS largest jobs bound any partition of the
        layers — also the one `project_grads` forms from the layers that have a gradient."""
        per_job = []
        for i in range(len(self.params)):
            need = int(TF.lib().t2v_sn_ws_floats(self._jobs([i]), 1))
            if need < 0:
                raise T2VError('t2v_sn_ws_floats failed with status %d' % need)
            per_job.append(need)
        worst = sum(sorted(per_job, reverse=True)[:SN_MAX_JOBS])
        self._ws = torch.empty(worst, dtype=torch.float32, device=self.params[0].device)

    def _launch_refresh(self, n_iter, from_param):
        if self._refresh_calls is None:
            self._refresh_calls = self._calls(list(range(len(self.params))))
        l, st = TF.lib(), TF._stream()
        for arr, n, _ in self._refresh_calls:
            TF.check(l.t2v_sn_refresh(arr, n, TF._p(self._ws), self._ws.numel(), n_iter, self.eps, 1 if from_param else 0, st),
                     't2v_sn_refresh')

    # ---- hot path (called by the optimiser) ------------------------------------------------------------------------------------
    def project_grads(self):
        """dL/dWhat -> dL/dW in place in every `weight.grad`, and `weight` <- W for the update that follows. Call when the
        gradients are complete (after the sink's flush and the data-parallel exchange: the map is linear and u, v, sigma, What are
        the same on every rank). Capturable."""
        grads = [p.grad for p in self.params]
        have = [i for i, g in enumerate(grads) if g is not None]
        for i in have:
            g, p = grads[i], self.params[i]
            if g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape or not g.is_contiguous():
                raise ValueError('the gradient of %s is not a contiguous fp32 tensor like its weight' % self.names[i])
        sig = tuple(g.data_ptr() if g is not None else 0 for g in grads)
        if self._project_sig != sig:
            self._project_calls = self._calls(have, grads) if have else []
            self._project_sig = sig
        l, st = TF.lib(), TF._stream()
        for arr, n, _ in self._project_calls:
            TF.check(l.t2v_sn_project(arr, n, TF._p(self._ws), self._ws.numel(), 1, st), 't2v_sn_project')
        for i, g in enumerate(grads):
            if g is None:                          # no gradient this step (the optimiser skips it too): only W goes back
                TF.copy_into(self.orig[i], self.params[i].detach())

    def refresh(self, touched=()):
        """`weight` holds the updated W: save it, `n_power_iterations` power iterations, `weight` <- W / sigma. Returns `touched`
        (the parameters the optimiser updated) extended by every normalised weight that is not in it: all of them were rewritten,
        so the optimiser re-packs all of them right behind this call. Capturable."""
        self._launch_refresh(self.n_iter, from_param=True)
        self.refreshes += 1
        seen = {id(p) for p in touched}
        return list(touched) + [p for p in self.params if id(p) not in seen]

    # ---- logging / tests ---------------------------------------------------------------------------------------------------
    def sigmas(self):
        """{state key: sigma} as Python floats (a host sync)."""
        return OrderedDict((k, float(s.item())) for k, s in zip(self.names, self.sigma))

    @property
    def launches_per_update(self):
        """Launches one discriminator update adds: the projection's 3 and the refresh's 5 n_power_iterations + 1 per call."""
        calls = (len(self.params) + SN_MAX_JOBS - 1) // SN_MAX_JOBS
        return calls * (3 + 5 * self.n_iter + 1)

    # ---- checkpoints ----------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """{'<key>_orig': W, '<key>_u': u, '<key>_v': v, '<key>_sigma': sigma} for every normalised weight."""
        out = OrderedDict()
        for k, w, u, v, s in zip(self.names, self.orig, self.u, self.v, self.sigma):
            for suffix, t in zip(STATE_SUFFIXES, (w, u, v, s)):
                out[k + suffix] = t.detach()
        return out

    @torch.no_grad()
    def load_state_dict(self, state):
        want = [k + s for k in self.names for s in STATE_SUFFIXES]
        missing = [k for k in want if k not in state]
        unknown = sorted(set(state) - set(want))
        if missing or unknown:
            raise KeyError('spectral-norm state does not match the discriminators: missing %s, unknown %s'
                           % (missing[:4], unknown[:4]))
        for k, w, u, v, s in zip(self.names, self.orig, self.u, self.v, self.sigma):
            for suffix, t in zip(STATE_SUFFIXES, (w, u, v, s)):
                src = state[k + suffix]
                if tuple(src.shape) != tuple(t.shape):
                    raise ValueError('%s has shape %s in the checkpoint, %s here' % (k + suffix, tuple(src.shape), tuple(t.shape)))
                t.copy_(src)


def check_checkpoint(to_load, enabled, path='the checkpoint'):
    """A checkpoint written with --D_sn holds W / sigma in its discriminator weights: without --D_sn the run would train those as
    plain weights and drop the master copies. Returns the spectral-norm state (None for a checkpoint without one)."""
    state = to_load.get('discrim_sn')
    if state is not None and not enabled:
        raise ValueError('%s was written with --D_sn (its discriminator weights are W / sigma and it carries the spectral-norm '
                         'state): pass --D_sn to continue from it' % path)
    return state


def check_flags(args):
    if getattr(args, 'D_sn', False) and getattr(args, 'end2end', False):
        raise NotImplementedError('--D_sn with --end2end: the text encoder shares the discriminator optimiser and its gradients '
                                  'bypass the gradient sink')


def attach(gan, optD, sn):
    """Make `sn` the spectral normalisation of `gan.discrims`: checkpoints carry its state, `optD` calls it around every update."""
    gan.discrim_sn = sn
    optD.weight_hook = sn
