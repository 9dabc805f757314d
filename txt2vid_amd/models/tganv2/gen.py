"""TGANv2 multi-scale generator (unconditional) — same surface / state_dict as
txt2vid/models/tganv2/gen.py:7-119. One process drives one GPU, so the reference's per-block
`data_parallel` scatter/gather disappears (data parallelism is process-level, see txt2vid_amd.dist)."""
import torch
import torch.nn as nn

from .. import layers as L
from ..layers import UpBlock, RenderBlock, Subsample, Linear
from ..conv_lstm import ConvLSTM
from ..tgan.temporal_gen import FrameSeedGenerator


class BaseFrameGen(nn.Module):
    """Three UpBlocks 1024 -> 512 -> 256 -> 128 (frames 1x1 -> 8x8); parameter names `up0..up2` as in the reference."""
    WIDTHS = (512, 256)

    def __init__(self, in_channels=1024, out_channels=128):
        super().__init__()
        self.out_channels = 128
        chain = (in_channels,) + self.WIDTHS + (out_channels,)
        for i, (cin, cout) in enumerate(zip(chain[:-1], chain[1:])):
            setattr(self, 'up%d' % i, UpBlock(in_channels=cin, out_channels=cout))

    def forward(self, x, cond=None, mod=None):
        """`mod`: the conditional modulation of the six BatchNorm sites for this forward (two per UpBlock, in order), or None."""
        for i in range(len(self.WIDTHS) + 1):
            x = getattr(self, 'up%d' % i)(x, mod=None if mod is None else mod[2 * i:2 * i + 2])
        return x


class CondModulation(nn.Module):
    """The projection of conditional BatchNorm (`MultiScaleGen(cond_bn=True)`, not in the reference): `weight` [2·ΣC, d] and
    `bias` [2·ΣC] map the condition vector to the (Δγ | Δβ) of every BatchNorm site of the generator. Both start as zeros and
    `init()` walks past this class without drawing, so a fresh cond_bn generator computes what the plain one computes and
    every other layer's host draws are unchanged."""

    def __init__(self, in_features, channels):
        super().__init__()
        self.in_features, self.channels = int(in_features), tuple(int(c) for c in channels)
        self.offsets = tuple(2 * sum(self.channels[:k]) for k in range(len(self.channels)))
        total = 2 * sum(self.channels)
        self.weight = nn.Parameter(torch.zeros(total, self.in_features))
        self.bias = nn.Parameter(torch.zeros(total))

    def forward(self, cond):
        from ...functional_cbn import table
        return table(cond, self.weight, self.bias, len(self.channels))


class MultiScaleGen(nn.Module):
    _cond_variant = False

    def __init__(self, latent_size=256, width=128, height=128, num_channels=3, additional_blocks=[64, 32, 32],
                 fm_channels=1024, num_frames=16, cond_dim=0, no_lstm=False, ca_dim=0, ca_kl_coeff=2.0, cond_bn=False):
        super().__init__()
        # cond_bn: every BatchNorm2d becomes a conditional site modulated by a projection of the condition vector
        # (functional_cbn.py; not in the reference, off by default). cond_bn = False builds exactly the reference's module.
        self.cond_bn_on = bool(cond_bn)
        if self.cond_bn_on and not self._cond_variant:
            raise ValueError('cond_bn (conditional BatchNorm) needs the text-conditioned generator '
                             'txt2vid.models.tganv2_cond.gen.MultiScaleGen')
        if self.cond_bn_on and cond_dim < 1:
            raise ValueError('cond_bn (conditional BatchNorm) needs a sentence code (cond_dim > 0): it cannot run with '
                             '--dont_use_sent')
        # ca_dim > 0: StackGAN++ conditioning augmentation turns the sentence code into c [B, ca_dim] in front of fc (models/ca.py;
        # not in the reference, off by default). ca_dim = 0 builds exactly the reference's module.
        self.ca_dim, self.ca_kl_coeff = int(ca_dim), float(ca_kl_coeff)
        if self.ca_dim < 0:
            raise ValueError('ca_dim must be >= 0 (got %d)' % self.ca_dim)
        if self.ca_dim and not self._cond_variant:
            raise ValueError('ca_dim > 0 (conditioning augmentation) needs the text-conditioned generator '
                             'txt2vid.models.tganv2_cond.gen.MultiScaleGen')
        if self.ca_dim and cond_dim < 1:
            raise ValueError('ca_dim > 0 (conditioning augmentation) needs a sentence code (cond_dim > 0): it cannot run with '
                             '--dont_use_sent')
        self.subsample = Subsample()
        # the recurrent state is a [fm_channels, height/64, width/64] map per sample: 1x1 for 64x64 frames, 2x2 for 128x128
        self.latent_size, self.fm_channels, self.latent_plane_ch = latent_size, fm_channels, fm_channels
        self.fm_width, self.fm_height = max(1, width // 64), max(1, height // 64)
        self.fm_size = self.latent_plane_ch * self.fm_height * self.fm_width
        if self.ca_dim:
            from ..ca import CondAugmentation
            self.ca = CondAugmentation(cond_dim, self.ca_dim)
        self.fc = Linear(latent_size + ((self.ca_dim or cond_dim) if self._cond_variant else 0), self.fm_size)
        self.no_lstm = no_lstm
        if no_lstm:
            # TGAN-v1's frame-seed generator instead of the ConvLSTM: always 16 frames, whatever num_frames says (gen.py:40-43)
            self.frame_seed_gen = FrameSeedGenerator(self.fm_size, self.fm_size)
        else:
            self.clstm = ConvLSTM(input_channels=fm_channels, hidden_channels=[fm_channels], kernel_size=3, step=num_frames,
                                  effective_step=range(num_frames))
        # level 0 = BaseFrameGen (-> 128 channels), then one UpBlock per entry of additional_blocks; a RenderBlock per level.
        # The text-conditioned variant puts its 2-D non-local block into the last-but-one UpBlock.
        widths = [128] + list(additional_blocks)
        nl_at = len(additional_blocks) - 1 if self._cond_variant else -1
        levels = [BaseFrameGen()]
        levels += [UpBlock(in_channels=widths[i - 1], out_channels=widths[i], with_non_local=(i == nl_at)) for i in range(1, len(widths))]
        self.abstract_blocks = nn.ModuleList(levels)
        self.render_blocks = nn.ModuleList([RenderBlock(in_channels=w, out_channels=num_channels) for w in widths])
        if self.cond_bn_on:
            # registered after every BatchNorm: the sites are the BatchNorm2d modules in registration order
            self.cond_bn = CondModulation(self.ca_dim or cond_dim, [m.num_features for m in self.cond_bn_sites()])
        for weight, taps in self.structurally_live_taps().items():
            weight._t2v_live_taps = list(taps)          # the optimiser only walks these taps of the (tap-major) master copies

    def cond_bn_sites(self):
        """The BatchNorm2d modules in registration order: site k of conditional BatchNorm (six in BaseFrameGen, two per later
        UpBlock, then one per RenderBlock)."""
        return [m for m in self.modules() if isinstance(m, L.BatchNorm2d)]

    def cond_bn_table(self):
        """[(k, C_k, o_k)]: site, channels, first column in the table [B, 2·ΣC]."""
        if not self.cond_bn_on:
            return []
        return [(k, c, o) for k, (c, o) in enumerate(zip(self.cond_bn.channels, self.cond_bn.offsets))]

    def structurally_live_taps(self):
        """{weight: live kernel taps} for the ConvLSTM when its state is 1x1 (frames below 128x128): a 3x3 kernel on a 1x1
        map only ever multiplies — and only ever receives a gradient through — its centre tap. Used by `dist.model_arena`:
        8 x [1024,1024,3,3] weights = 302 MB of gradients of which 33.5 MB can be non-zero."""
        if self.no_lstm or self.fm_width != 1 or self.fm_height != 1:
            return {}
        cell = self.clstm.cell0
        k = cell.kernel_size
        centre = (k // 2) * k + k // 2
        return {m.weight: [centre] for m in (cell.Wxi, cell.Wxf, cell.Wxc, cell.Wxo, cell.Whi, cell.Whf, cell.Whc, cell.Who)}

    def load_state_dict(self, state_dict, strict=True, **kw):
        """A checkpoint written with conditioning augmentation (`ca.fc.*` keys) loads only into a generator built with the same
        ca_dim, and one without into one without: a clear error instead of a bare shape mismatch on fc.weight."""
        w = state_dict.get('ca.fc.weight')
        got = 0 if w is None else int(w.shape[0]) // 4
        if got != self.ca_dim:
            raise ValueError('generator checkpoint %s conditioning augmentation (ca_dim=%d) but this generator was built with '
                             'ca_dim=%d: pass the same ca_dim in the --G spec' % ('has' if got else 'has no', got, self.ca_dim))
        has = 'cond_bn.weight' in state_dict
        if has != self.cond_bn_on:
            raise ValueError('generator checkpoint %s conditional BatchNorm (cond_bn.* keys) but this generator was built with '
                             'cond_bn=%s: pass the same cond_bn in the --G spec' % ('has' if has else 'has no', self.cond_bn_on))
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def forward(self, x, cond=None, return_abstract_maps=False, output_blocks=None, return_kl=False):
        """`return_kl`: also return the conditioning augmentation's KL term (a 0-d device tensor; None without CA) as the last
        element: (rendered, kl) or (rendered, abstract, kl)."""
        from ... import functional as TF
        kl = None
        if self.cond_bn_on and cond is None:
            raise ValueError('conditional BatchNorm (cond_bn) needs the sentence code')
        latent = x.size(1)
        if self.ca_dim:
            if cond is None:
                raise ValueError('conditioning augmentation (ca_dim=%d) needs the sentence code' % self.ca_dim)
            x, kl = self.ca(x, cond)                           # [z | c] in one launch, eps drawn before the Subsample phases
            if self.cond_bn_on:
                # [z | c] feeds fc and (its c columns) the projection: a grouped fork sums the two gradients in one launch
                (x,), (xc,) = TF.fork_group([x])
                vec = TF.SliceCols.apply(xc, latent, self.ca_dim)
        elif cond is not None:
            if self.cond_bn_on:
                (cond,), (vec,) = TF.fork_group([cond])        # (aliases only where the sentence code carries a gradient: --end2end)
            x = TF.cat_features(x, cond)
        mod = self.cond_bn(vec) if self.cond_bn_on else None
        x = self.fc(x)
        if self.no_lstm:
            # [B, fm, 16] contiguous; the reference's view(B, 16, -1, h, w) + merge_frames reinterprets that memory as
            # [B*16, C, h, w] (channels and frames scrambled on purpose: no permute)
            x = self.frame_seed_gen(x)
            num_frames = 16
            x = x.view(x.size(0) * num_frames, -1, self.fm_height, self.fm_width)
        else:
            x = x.view(x.size(0), self.latent_plane_ch, self.fm_height, self.fm_width)
            hs = self.clstm.forward_stacked(x)                 # [T,B,C,h,w]
            num_frames = hs.size(0)
            x = TF.time_to_batch(hs)                           # [B*T,C,h,w]  (stack+permute+merge_frames)

        abstract, rendered = [], []
        n_levels = len(self.render_blocks)
        stride = 1                                     # level sample j is base sample j * stride (Subsample keeps ::2 per level)

        def sites(ks):
            if mod is None:
                return None
            return [mod.site(self.cond_bn.offsets[k], stride, num_frames) for k in ks]
        for i in range(n_levels):
            if i != 0 and self.training:
                # [b*T,C,h,w] -> subsample batch and time -> [ceil(b/2)*T/2, C, h, w]
                x, _ = self.subsample_frames(x, num_frames)
                num_frames //= 2
                stride *= 2
            x = self.abstract_blocks[i](x, mod=sites(range(6) if i == 0 else (4 + 2 * i, 5 + 2 * i)))
            abstract.append(x)
            if i == n_levels - 1 or self.training or (output_blocks is not None and i in output_blocks):
                rmod = None if mod is None else sites([4 + 2 * n_levels + i])[0]
                if i + 1 < n_levels:
                    r, x = self.render_blocks[i](x, fork=True, mod=rmod)     # the map also feeds the next level
                else:
                    r = self.render_blocks[i](x, mod=rmod)
                rendered.append(TF.frames_to_video(r, num_frames))           # [b,C,T,H,W]
        if return_abstract_maps:
            return (rendered, abstract, kl) if return_kl else (rendered, abstract)
        return (rendered, kl) if return_kl else rendered

    def subsample_frames(self, x, num_frames):
        """`Subsample` applied on the merged-frames layout: keeps samples ::2 and frames bt::2
        (gen.py:98-106). bt is drawn from the CPU generator exactly like the reference."""
        from ... import functional as TF
        bt, bt_dev = TF.draws.phase()
        return TF.subsample_frames(x, num_frames, bt, bt_dev), bt
