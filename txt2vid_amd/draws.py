"""Random draws of one training iteration, made on the HOST generators in the reference's order (RNG parity); see
`txt2vid_amd.functional.draws` / `set_draws` for the instance the ops read."""
import torch


# ------------------------------------------------------------------------------------------------
# random draws of one training iteration (SURVEY §7 "RNG parity"): always made on the HOST generators in
# the reference's order. `HostDraws` hands them out as they are made (eager mode); `StaticDraws` makes
# all of an iteration's draws up front and keeps them in fixed device buffers, so that a captured HIP
# graph reads this iteration's phases / z / alphas from the same addresses on every replay.
# ------------------------------------------------------------------------------------------------

AUG_K = 8           # uniforms per sample of one augmentation block (functional_aug.K)


class HostDraws(object):
    def multiscale_t0(self, n):
        """n Subsample draws of trainer.multiscale_data; returns per level (t0 host int, None)."""
        out, t0, st = [], 0, 1
        for _ in range(n):
            out.append((t0, None))
            bt = int(torch.randint(2, (1,)))
            t0, st = t0 + bt * st, st * 2
        return out

    def phase(self):
        return int(torch.randint(2, (1,))), None

    def z(self, batch, latent, device):
        return torch.randn(batch, latent).to(device, non_blocking=True)

    def alpha(self, b, ndim, device):
        return torch.rand(b, *([1] * (ndim - 1))).reshape(b).to(device=device, dtype=torch.float32)

    def ca_eps(self, b, d, device):
        """eps ~ N(0, 1) [b, d] of the generator's conditioning augmentation (one draw per generator forward, like z)."""
        return torch.randn(b, d).to(device, non_blocking=True)

    def aug(self, b, device, gated=False, geo=False):
        """One block u [b, AUG_K] of uniforms for an augmentation of D's inputs (functional_aug), drawn when it is consumed.
        `gated` (adaptive strength): (u, g), the gate block g [b, AUG_K] drawn immediately after u. `geo` (a policy
        with a geometric name): one more block v [b, AUG_K] drawn behind them, (u, v) or (u, g, v)."""
        u = torch.rand(b, AUG_K).to(device, non_blocking=True)
        if not gated and not geo:
            return u
        out = (u,)
        if gated:
            out += (torch.rand(b, AUG_K).to(device, non_blocking=True),)
        if geo:
            out += (torch.rand(b, AUG_K).to(device, non_blocking=True),)
        return out

    def perm(self, n, device):
        """A non-identity permutation of range(n) from numpy's global RNG (util/misc.gen_perm), as a device int32 tensor."""
        import numpy as _np
        from .util.misc import gen_perm
        return torch.from_numpy(_np.ascontiguousarray(gen_perm(n), dtype=_np.int32)).to(device)


class StaticDraws(object):
    def __init__(self, device, batch, latent, n_levels, n_gen_phases=3, gp=True, subsample_input=True, n_perms=0,
                 n_d_steps=1, n_g_steps=1, ca_dim=0, n_aug=0, n_geo=0):
        self.n_perms = n_perms                      # caption permutations per iteration (conditional path: D steps, real_pred)
        self.n_d_steps, self.n_g_steps = n_d_steps, n_g_steps     # one set of GP alphas per D step, of G phases per G forward
        self._p = 0
        self.device, self.batch, self.latent = device, batch, latent
        self.ca_dim = ca_dim                        # conditioning augmentation: one eps [batch, ca_dim] per G forward (0: none)
        self.n_levels, self.n_gen, self.gp, self.sub = n_levels, n_gen_phases, gp, subsample_input
        # augmentation of D's inputs (--D_aug): blocks [batch, AUG_K] per iteration, in the eager order of consumption — a real and
        # a generated block per D step and at G part 0, a generated block per later G step (0: none, today's layout). With gated
        # augmentation (adaptive strength) twice as many: every parameter block is followed by its gate block
        if n_aug not in (0, 2 * n_d_steps + n_g_steps + 1, 2 * (2 * n_d_steps + n_g_steps + 1)):
            raise ValueError('an iteration of %d D and %d G steps consumes %d augmentation blocks (twice as many with gates), not %d'
                             % (n_d_steps, n_g_steps, 2 * n_d_steps + n_g_steps + 1, n_aug))
        # a policy with a geometric name: one more block v behind every u (and its g), 2N + M + 1 of them (0: none)
        if n_geo not in (0, 2 * n_d_steps + n_g_steps + 1) or (n_geo and not n_aug):
            raise ValueError('an iteration of %d D and %d G steps consumes %d geometric blocks, each behind an augmentation block, '
                             'not %d' % (n_d_steps, n_g_steps, 2 * n_d_steps + n_g_steps + 1, n_geo))
        self.n_aug, self.n_geo = n_aug, n_geo
        self.gated = n_aug > 2 * n_d_steps + n_g_steps + 1
        self.geo = n_geo > 0
        self._w = 1 + int(self.gated) + int(self.geo)     # blocks per draw: u, its gate block g, its geometric block v, in a row
        self.bs = [batch]
        for _ in range(n_levels - 1):
            self.bs.append((self.bs[-1] + 1) // 2)
        # one pinned staging buffer and one device buffer of 32-bit words for every draw of an iteration (int32 phases |
        # float32 z | float32 alphas | int32 caption permutations | float32 CA eps of every G forward, absent without CA | float32
        # augmentation blocks, absent without --D_aug): ONE H2D
        # copy node per replayed iteration instead of four (a copy node costs ~20 us of idle time in the replayed graph)
        n_int, n_z, n_a, n_p = n_levels + n_gen_phases * n_g_steps, batch * latent, sum(self.bs) * n_d_steps, max(1, n_perms) * batch
        n_e = batch * ca_dim * n_g_steps
        n_u = batch * AUG_K * (n_aug + n_geo)
        # The staging side is a RING of pinned buffers: the upload is asynchronous and the training loop runs the host ahead of
        # the GPU (losses are read one iteration late), so a single staging buffer would be rewritten with iteration i + 1's draws
        # before the copy of iteration i has executed. A slot is reused only after the event behind its last copy has completed.
        self.RING = 4
        on_gpu = torch.device(device).type != 'cpu'        # (a CPU "device": the host-side draw order alone, no pinned memory)
        self.h_ring = [torch.zeros(n_int + n_z + n_a + n_p + n_e + n_u, dtype=torch.int32) for _ in range(self.RING)]
        if on_gpu:
            self.h_ring = [h.pin_memory() for h in self.h_ring]
        self.h_events = [None] * self.RING
        self._slot = 0
        self.h_all = self.h_ring[0]
        self.d_all = self.h_all.to(device) if on_gpu else self.h_all.clone()     # (zeros by copy: a memcpy, no fill kernel)

        def carve(buf):
            o = 0
            i_ = buf[o:o + n_int]; o += n_int
            z_ = buf[o:o + n_z].view(torch.float32).view(batch, latent); o += n_z
            a_ = buf[o:o + n_a].view(torch.float32); o += n_a
            p_ = buf[o:o + n_p].view(max(1, n_perms), batch); o += n_p
            e_ = buf[o:o + n_e].view(torch.float32).view(n_g_steps, batch, ca_dim) if n_e else None
            o += n_e
            u_ = buf[o:o + n_u].view(torch.float32).view(n_aug + n_geo, batch, AUG_K) if n_u else None
            return i_, z_, a_, p_, e_, u_
        self._carve = carve
        self.h_int, self.h_z, self.h_a, self.h_perm, self.h_eps, self.h_u = carve(self.h_all)
        self.d_int, self.d_z, self.d_a, self.d_perm, self.d_eps, self.d_u = carve(self.d_all)
        self._i = self._a = self._e = self._u = 0

    def begin_step(self):
        """All host draws of one iteration, reference order (trainer.py:221-263): n_levels Subsample phases, z, the generator's
        phases of its first forward, the GP alphas per level of every D step, the generator's phases of every later G
        forward; numpy: the caption permutations in the order they are consumed. Then one small H2D copy on the current
        stream. With conditioning augmentation every G forward draws its eps first, in front of its phases: z, eps 0, phases 0,
        alphas, then eps j, phases j for each later forward j. With augmentation of D's inputs every D step draws a real and a
        generated block in front of its alphas, G part 0 draws a real and a generated block behind the last D step, and every later
        G forward j draws a generated block behind its phases. With gated augmentation every one of these blocks u is followed at
        once by its gate block g (u, g, u, g, ...), next to it in the staging buffer. With a geometric policy every one of them is
        followed, behind its gate block if it has one, by its geometric block v (u, [g], v, u, [g], v, ...), in the same buffer."""
        slot = self._slot
        self._slot = (slot + 1) % self.RING
        if self.h_events[slot] is not None:
            self.h_events[slot].synchronize()            # (the copy that last read this slot is done; normally long ago)
        self.h_all = self.h_ring[slot]
        self.h_int, self.h_z, self.h_a, self.h_perm, self.h_eps, self.h_u = self._carve(self.h_all)
        t0, st = 0, 1
        for l in range(self.n_levels):
            self.h_int[l] = t0
            if self.sub:
                bt = int(torch.randint(2, (1,)))
                t0, st = t0 + bt * st, st * 2
        self.h_z.copy_(torch.randn(self.batch, self.latent))
        if self.ca_dim:
            self.h_eps[0].copy_(torch.randn(self.batch, self.ca_dim))
        for k in range(self.n_gen):
            self.h_int[self.n_levels + k] = int(torch.randint(2, (1,)))
        off = blk = 0
        for _ in range(self.n_d_steps):
            if self.n_aug:
                for _ in range(2 * self._w):
                    self.h_u[blk].copy_(torch.rand(self.batch, AUG_K))
                    blk += 1
            if self.gp:
                for b in self.bs:
                    self.h_a[off:off + b] = torch.rand(b, 1, 1, 1, 1).reshape(b)
                    off += b
        if self.n_aug:
            for _ in range(2 * self._w):
                self.h_u[blk].copy_(torch.rand(self.batch, AUG_K))
                blk += 1
        for j in range(1, self.n_g_steps):
            if self.ca_dim:
                self.h_eps[j].copy_(torch.randn(self.batch, self.ca_dim))
            for k in range(self.n_gen * j, self.n_gen * (j + 1)):
                self.h_int[self.n_levels + k] = int(torch.randint(2, (1,)))
            if self.n_aug:
                for _ in range(self._w):
                    self.h_u[blk].copy_(torch.rand(self.batch, AUG_K))
                    blk += 1
        if self.n_perms:
            from .util.misc import gen_perm
            for k in range(self.n_perms):
                self.h_perm[k].copy_(torch.from_numpy(gen_perm(self.batch).astype('int32')))
        if self.d_all.is_cuda:
            # a copy KERNEL reading the pinned buffer in place (pinned host memory is mapped into the device's address space): it
            # stays on the compute queue, where the copy engine's memcpy costs a queue hand-over each way in front of the graph
            # that reads the draws (~100 us of idle time per iteration in the text-conditioned loop, ~20 us in the unconditional one)
            from . import functional as TF
            TF._copy2d(self.h_all, 0, self.h_all.numel(), self.d_all, 0, self.h_all.numel(), 1, self.h_all.numel())
        else:
            self.d_all.copy_(self.h_all, non_blocking=True)
        if self.d_all.is_cuda:
            ev = torch.cuda.Event()
            ev.record()
            self.h_events[slot] = ev
        self._i = self._a = self._p = self._e = self._u = 0

    def multiscale_t0(self, n):
        assert n == self.n_levels
        return [(0, self.d_int[l:l + 1]) for l in range(n)]

    def phase(self):
        k = self._i
        self._i += 1
        return 0, self.d_int[self.n_levels + k:self.n_levels + k + 1]

    def z(self, batch, latent, device):
        return self.d_z

    def alpha(self, b, ndim, device):
        off = self._a
        self._a += b
        return self.d_a[off:off + b]

    def perm(self, n, device):
        assert n == self.batch and self._p < self.n_perms
        k = self._p
        self._p += 1
        return self.d_perm[k]

    def ca_eps(self, b, d, device):
        assert b == self.batch and d == self.ca_dim and self._e < self.n_g_steps
        k = self._e
        self._e += 1
        return self.d_eps[k]

    def aug(self, b, device, gated=False, geo=False):
        assert b == self.batch and self._u < self.n_aug + self.n_geo and bool(gated) == self.gated and bool(geo) == self.geo
        k = self._u
        self._u += self._w
        return tuple(self.d_u[k + i] for i in range(self._w)) if self._w > 1 else self.d_u[k]

    def rewind(self):
        self._i = self._a = self._p = self._e = self._u = 0
