"""3-D ResNet discriminator trunk with a non-local block and un/conditional heads — same surface and
state_dict as txt2vid/models/resnet3d.py:6-57, every op a gfx950 kernel."""
import torch
import torch.nn as nn

from .. import functional as TF
from .layers import ResidualBlock, DownBlock, Attention3d, Conv3d, AvgPool3d, ReLU, Linear, down_block_levels, nonlocal_levels


_PROJ_MISMATCH = ('discriminator checkpoint %s projection head (proj.weight key) but this discriminator was built with proj=%s: '
                  'pass the same proj in the --D spec')


_MBSTD_MISMATCH = ('discriminator checkpoint %s minibatch standard deviation head (mbstd.weight key) but this discriminator was '
                   'built with mbstd=%s: pass the same mbstd in the --D spec')


_MATCH_MISMATCH = ('discriminator checkpoint %s matching head (match.weight key) but this discriminator was built with match=%s: '
                   'pass the same match in the --D spec')

MATCH_SEED = 0x6d617463           # the draws of every matching head's initial W: a generator of its own under this constant


class MinibatchStd(nn.Module):
    """The weight of the minibatch standard deviation head (`Resnet3D(mbstd=G)`, Karras et al. 2018; not in the reference). One
    definition (functional_mbstd.py): rows [i·seg, (i+1)·seg) of the features f [b, K] form a segment (seg = b unless stated),
    runs of G consecutive rows inside a segment a group, the last one holding the remainder; per group q of n rows
    σ_k = sqrt((1/n) Σ_b (f_bk − μ_k)² + 1e-8), s_q = (1/K) Σ_k σ_k, and the logits of the group's rows gain w_u·s_q
    (unconditional) and w_c·s_q (conditional). `weight` = w = (w_u, w_c), or (w_u,) without a sentence code: StyleGAN's extra
    feature column in front of the linear heads. w starts as zeros and `init()` walks past this class without drawing, so a
    fresh model computes what the plain one computes and every other layer's host draws are unchanged; dL/dw is not zero
    there, so training moves it. Not an nn.Linear: `--D_sn` leaves w alone."""

    def __init__(self, group, heads):
        super().__init__()
        self.group = TF.mbstd_check_group(group)
        self.weight = nn.Parameter(torch.zeros(int(heads)))

    def forward(self, feats, us, cs, segs=None):
        """(us, cs) with the term added, one launch for every member and both heads; a head given as None is not computed."""
        bases = [us, cs][:self.weight.numel()]
        res = TF.mbstd_group(self.weight, self.group, feats, bases, segs)
        return res[0], (res[1] if len(res) > 1 else cs)


class CondProjection(nn.Module):
    """The weight of the projection head (`Resnet3D(proj=True)`, Miyato & Koyama 2018; not in the reference): `weight` = V
    [in_ch, cond_dim] adds featᵀ V s to the conditional logit (functional_proj.py). V starts as zeros and `init()` walks past
    this class without drawing, so a fresh proj discriminator computes what the plain one computes and every other layer's host
    draws are unchanged; dL/dV is not zero there, so training moves it. Not an nn.Linear: `--D_sn` leaves V alone."""

    def __init__(self, in_features, cond_dim):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(int(in_features), int(cond_dim)))

    def forward(self, feats, conds, bases):
        """bases[i] + ((feats[i] @ V) * conds[i]).sum(1, keepdim=True) for every member, one launch."""
        return TF.proj_rows_group(self.weight, feats, conds, bases)


class CondMatch(nn.Module):
    """The weight of the matching head (`Resnet3D(match=True)`, XMC-GAN, Zhang et al. 2021; not in the reference): `weight` = W
    [in_ch, cond_dim] embeds the trunk's features next to the sentence codes for the contrastive clip-caption term of
    `--D_match` / `--G_match` (functional_match.py). The head never feeds a logit: a match discriminator outputs what the plain
    one outputs, bit for bit. W cannot start at zero (the cosine has no gradient direction there): it is drawn as N(0, 1/in_ch)
    from a torch.Generator of its own under MATCH_SEED, and `init()` walks past this class without drawing, so every other
    layer's host draws are unchanged. Not an nn.Linear: `--D_sn` leaves W alone. `ones` (not in the state dict) is the constant
    vector the embedding launch takes as its row weights: made here, outside any graph capture."""

    def __init__(self, in_features, cond_dim):
        super().__init__()
        g = torch.Generator()
        g.manual_seed(MATCH_SEED)
        self.weight = nn.Parameter(torch.randn(int(in_features), int(cond_dim), generator=g) * (1.0 / int(in_features)) ** 0.5)
        self.register_buffer('ones', torch.ones(TF.MATCH_MAX_ROWS), persistent=False)

    def forward(self, feats, conds, tau, stats, frozen=False):
        """The mean over the members of the matching term of (feats[i] @ W, conds[i]) as a 0-d tensor: two launches. `frozen`:
        W is a constant of this call (the G step, where D's parameters get no gradient)."""
        return TF.match_group(self.weight.detach() if frozen else self.weight, feats, conds, tau, stats, ones=self.ones)


class Resnet3D(nn.Module):

    def __init__(self, num_channels=1, mid_ch=64, which_conv=None, which_pool=None, cond_dim=0, num_down_blocks=4,
                 wide=False, with_attn=True, proj=False, mbstd=0, match=False):
        super().__init__()
        # proj: the conditional logit gains the bilinear term featᵀ V s of a projection discriminator (functional_proj.py; not in
        # the reference, off by default). proj = False builds exactly the reference's module.
        if proj and cond_dim < 1:
            raise ValueError('proj (projection head) needs a sentence code (cond_dim > 0): it cannot run with --dont_use_sent')
        # match: the head of the contrastive clip-caption matching term (CondMatch above; not in the reference, off by default).
        # match = False builds exactly the reference's module.
        if match and cond_dim < 1:
            raise ValueError('match (matching head) needs a sentence code (cond_dim > 0): it cannot run with --dont_use_sent')
        # mbstd: group size G of the minibatch standard deviation head (MinibatchStd above; not in the reference); 0 = off builds
        # exactly the reference's module.
        if mbstd != 0:
            TF.mbstd_check_group(mbstd)
        which_conv = which_conv or Conv3d
        which_pool = which_pool or AvgPool3d
        self.activation = ReLU()
        res_path = nn.Sequential(which_conv(num_channels, mid_ch, 3, 1, padding=1), self.activation,
                                 which_conv(mid_ch, mid_ch, 3, 1, padding=1), which_pool((1, 2, 2), 2))
        skip = nn.Sequential(which_pool((1, 2, 2), 2), which_conv(num_channels, mid_ch, 1))
        self.res_block = ResidualBlock(inner_module=res_path, identity_map=skip)
        down, in_ch, out_ch = [], mid_ch, 128
        for i in range(num_down_blocks):
            down.append(DownBlock(in_channels=in_ch, out_channels=out_ch, which_conv=which_conv, wide=wide))
            if i == 0 and with_attn:
                down.append(Attention3d(out_ch, which_conv=which_conv))
            in_ch, out_ch = out_ch, out_ch * 2
        self.down = nn.ModuleList(down)
        self.fc_uncond = Linear(in_ch, 1)
        if cond_dim > 0:
            self.fc = Linear(in_ch + cond_dim, 1)
        if proj:
            self.proj = CondProjection(in_ch, cond_dim)           # registered after fc: one trailing state-dict key
        if mbstd:
            self.mbstd = MinibatchStd(mbstd, 2 if cond_dim > 0 else 1)        # registered last: one trailing state-dict key
        if match:
            self.match = CondMatch(in_ch, cond_dim)               # registered last of all: one trailing state-dict key

    def groupable(self):
        m = self.res_block.inner_module
        return isinstance(m[0], Conv3d) and isinstance(m[2], Conv3d) and all(
            isinstance(d, (DownBlock, Attention3d)) for d in self.down)

    def forward_levels(self, xs, conds=None, segs=None):
        """All pyramid levels through the shared trunk in lock-step: every convolution layer is ONE grouped
        launch over the levels (same results as level-by-level `forward`, resnet3d.py:38-57). segs (mbstd only): the segment
        length of every member for the minibatch statistic (default: its batch size) — a real‖fake member of 2b rows takes b."""
        m = self.res_block.inner_module
        idm = self.res_block.identity_map
        # the clips feed the residual path and the skip path: a grouped fork sums their two gradients (generator step, gradient
        # penalty) in one launch for all levels instead of one autograd-engine add per level
        xs, xs_skip = TF.fork_group(xs)
        hs = TF.conv_group(xs, m[0].weight, m[0].bias)
        pool_h = None
        if isinstance(m[3], AvgPool3d) and isinstance(idm[0], AvgPool3d) and \
                (m[3].kernel_size, m[3].stride, m[3].padding) == ((1, 2, 2), (2, 2, 2), (0, 0, 0)) and TF.pool_conv_ok(hs, m[2].weight, True):
            # conv2 feeds ONLY the pooling: pool(conv3(relu(h))) = stride-2 conv3 of the box-summed activation — 27 taps over the
            # pooled voxels (a quarter of the even-frame MACs), same values up to summation order (functional_pool.py)
            zs = TF.pool_conv_group(hs, m[2].weight, m[2].bias, relu_in=True, stem=True)
            cfg_x = [(idm[0].kernel_size, idm[0].stride, idm[0].padding)] * len(xs)
            ss = TF.conv_group(TF.avg_pool3d_group(xs_skip, cfg_x), idm[1].weight, idm[1].bias)
            hs = TF.add_group(zs, ss)
            pool_h = False
        elif isinstance(m[3], AvgPool3d) and isinstance(idm[0], AvgPool3d):
            pool_h = (m[3].kernel_size, m[3].stride, m[3].padding)
            if pool_h[0][0] == 1 and pool_h[1][0] == 2 and pool_h[2][0] == 0 and TF.even_frames_ok(hs, m[2].weight):
                # AvgPool3d((1,2,2), stride 2) keeps the even frames of conv2 only: compute just those (half the forward GEMM)
                # and pool what is left with a frame stride of 1
                hs = TF.conv_even_frames_group(hs, m[2].weight, m[2].bias, relu_in=True)
                pool_h = (pool_h[0], (1,) + tuple(pool_h[1][1:]), pool_h[2])
            else:
                hs = TF.conv_group(hs, m[2].weight, m[2].bias, relu_in=True)
        else:
            hs = TF.conv_group(hs, m[2].weight, m[2].bias, relu_in=True)
        if pool_h is False:
            pass                                                                  # (pooled convolution above: already summed)
        elif pool_h is not None:
            cfg_h = [pool_h] * len(xs)
            cfg_x = [(idm[0].kernel_size, idm[0].stride, idm[0].padding)] * len(xs)
            ss = TF.conv_group(TF.avg_pool3d_group(xs_skip, cfg_x), idm[1].weight, idm[1].bias)
            hs = TF.avg_pool3d_group(hs, cfg_h, adds=ss)                       # pool + residual add, all levels, one launch
        else:
            ss = TF.conv_group([idm[0](x) for x in xs_skip], idm[1].weight, idm[1].bias)
            hs = [TF.add(s_, m[3](h)) for s_, h in zip(ss, hs)]
        for d in self.down:
            if isinstance(d, DownBlock):
                hs = down_block_levels(d, hs)
            else:
                hs = nonlocal_levels(d, hs)
        feats = TF.sum_spatial_group(hs)                                      # torch.sum(x, [2,3,4]) of every level: one launch
        f_u = f_c = feats
        mb = getattr(self, 'mbstd', None)
        f_m = None
        if mb is not None:
            # one more consumer of the features: the minibatch statistic (a grouped fork sums its gradient in one launch)
            f_m, rest = TF.fork_group(feats)
            if conds is None:
                f_u = rest
            else:
                feats = rest
        if conds is not None:
            # three consumers (unconditional head, conditional head, the caller's mismatched-caption head on the returned features):
            # two grouped forks sum their gradients for all levels in two launches instead of two ATen adds per level
            f_u, rest = TF.fork_group(feats)
            f_c, feats = TF.fork_group(rest)
        w5 = self.fc_uncond.weight.view(self.fc_uncond.weight.shape + (1, 1, 1))
        us = TF.conv_group([f.view(f.shape + (1, 1, 1)) for f in f_u], w5, self.fc_uncond.bias)   # all heads: one launch
        us = [u.view(u.shape[0], u.shape[1]) for u in us]
        if mb is None:
            cs = self.cond_heads(f_c, conds) if conds is not None else [None] * len(feats)
        elif conds is None:
            us, cs = mb(f_m, us, None, segs)[0], [None] * len(feats)
        else:
            us, cs = mb(f_m, us, self._cond_heads_plain(f_c, conds), segs)         # both heads of every member: one launch
        return [(u, c, feat) for feat, u, c in zip(feats, us, cs)]

    def cond_heads(self, feats, conds, segs=None):
        """`self.fc(torch.cat((features, cond), 1))` (resnet3d.py:53-55) for several levels / members at once: one launch for
        all concatenations, one for all heads (instead of two copies + one linear per member). With mbstd, plus w_c·s of every
        member's own rows (segs: a segment length per member, default its row count)."""
        mb = getattr(self, 'mbstd', None)
        if mb is None:
            return self._cond_heads_plain(feats, conds)
        feats, conds = list(feats), list(conds)
        if not (1 <= len(feats) <= TF.MAX_GROUPS) or not feats[0].is_cuda:
            return [self._cond_head(f, c, None if segs is None else segs[i]) for i, (f, c) in enumerate(zip(feats, conds))]
        feats, feats_m = TF.fork_group(feats)
        return mb(feats_m, None, self._cond_heads_plain(feats, conds), segs)[1]

    def _cond_heads_plain(self, feats, conds):
        """The conditional heads without the minibatch statistic."""
        feats, conds = list(feats), list(conds)
        proj = getattr(self, 'proj', None)
        if not (1 <= len(feats) <= TF.MAX_GROUPS) or not feats[0].is_cuda:
            return [self._cond_head_plain(f, c) for f, c in zip(feats, conds)]
        feats_p, conds_p = feats, conds
        if proj is not None:
            # features and sentence codes feed the existing head AND the projection term: grouped forks sum the two gradients of
            # all members in one launch each (tensors without a gradient pass through)
            feats, feats_p = TF.fork_group(feats)
            conds, conds_p = TF.fork_group(conds)
        cats = TF.cat_features_group(feats, conds)
        w5 = self.fc.weight.view(self.fc.weight.shape + (1, 1, 1))
        cs = TF.conv_group([c.view(c.shape + (1, 1, 1)) for c in cats], w5, self.fc.bias)
        cs = [c.view(c.shape[0], c.shape[1]) for c in cs]
        return cs if proj is None else proj(feats_p, conds_p, cs)

    def _cond_head(self, feat, cond, seg=None):
        """The conditional head of one member: the same values as `cond_heads` on a list of one."""
        mb = getattr(self, 'mbstd', None)
        if mb is None:
            return self._cond_head_plain(feat, cond)
        (f,), (f_m,) = TF.fork_group([feat])
        return mb([f_m], None, [self._cond_head_plain(f, cond)], None if seg is None else [seg])[1][0]

    def _cond_head_plain(self, feat, cond):
        proj = getattr(self, 'proj', None)
        if proj is None:
            return self.fc(TF.cat_features(feat, cond))
        (f, f_p), (s, s_p) = TF.fork_group([feat]), TF.fork_group([cond])
        return proj(f_p, s_p, [self.fc(TF.cat_features(f[0], s[0]))])[0]

    def load_state_dict(self, state_dict, strict=True, **kw):
        """A checkpoint written with the projection head (`proj.weight`) loads only into a trunk built with proj=True, and one
        without into one without: a clear error instead of a bare missing / unexpected key."""
        has = 'proj.weight' in state_dict
        if has != hasattr(self, 'proj'):
            raise ValueError(_PROJ_MISMATCH % ('has' if has else 'has no', hasattr(self, 'proj')))
        has = 'mbstd.weight' in state_dict
        if has != hasattr(self, 'mbstd'):
            raise ValueError(_MBSTD_MISMATCH % ('has' if has else 'has no', self.mbstd.group if hasattr(self, 'mbstd') else 0))
        has = 'match.weight' in state_dict
        if has != hasattr(self, 'match'):
            raise ValueError(_MATCH_MISMATCH % ('has' if has else 'has no', hasattr(self, 'match')))
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def forward(self, x=None, cond=None, xbar=None, computed_features=None, seg=None):
        """seg (mbstd only): the segment length of the rows for the minibatch statistic (default: all rows are one segment)."""
        uncond = None
        mb = getattr(self, 'mbstd', None)
        if computed_features is None and x is not None and self.groupable():
            # one tensor = a group of one: the same launches and the same fused adjoints (forked inputs, conv1 + skip in one
            # Function, grouped non-local block) as the multi-level pass
            if mb is not None:
                return self.forward_levels([x], [cond] if cond is not None else None, None if seg is None else [seg])[0]
            return self.forward_levels([x], [cond] if cond is not None else None)[0]
        if computed_features is not None:
            x = computed_features
        else:
            x = self.res_block(x)           # a trunk built from foreign layers: the plain module composition
            for d in self.down:
                x = d(x)
            x = TF.sum_spatial(x)                           # torch.sum(x, [2,3,4])  (resnet3d.py:48)
            computed_features = x
            if mb is None:
                uncond = self.fc_uncond(x)
            else:
                (f_u,), (f_m,) = TF.fork_group([x])
                uncond = mb([f_m], [self.fc_uncond(f_u)], None, None if seg is None else [seg])[0][0]
        if cond is not None:
            c = self._cond_head(x, cond, seg) if mb is not None else self._cond_head(x, cond)
            return uncond, c, computed_features
        return uncond, None, computed_features
