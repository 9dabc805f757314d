"""Multi-scale discriminator: one Resnet3D shared by the 4 pyramid levels —
txt2vid/models/tganv2/discrim.py:7-31 (state_dict keys `single_discrim.*`)."""
import torch.nn as nn

from ..resnet3d import Resnet3D, _PROJ_MISMATCH, _MBSTD_MISMATCH, _MATCH_MISMATCH
from ... import functional as TF


class MultiScaleDiscrim(nn.Module):
    _wrap = False

    def __init__(self, discrim_down_blocks=[4, 4, 4, 4], num_channels=3, cond_dim=0, underlying_discrim=Resnet3D,
                 single_discrim=True, proj=False, mbstd=0, match=False):
        super().__init__()
        # proj: the projection head of every underlying discriminator (models/resnet3d.py; not in the reference, off by default)
        self.proj_on = bool(proj)
        if self.proj_on and not self._wrap:
            raise ValueError('proj (projection head) needs the text-conditioned discriminator '
                             'txt2vid.models.tganv2_cond.discrim.MultiScaleDiscrim')
        if self.proj_on and cond_dim < 1:
            raise ValueError('proj (projection head) needs a sentence code (cond_dim > 0): it cannot run with --dont_use_sent')
        extra = {'proj': True} if self.proj_on else {}
        # mbstd: group size of the minibatch standard deviation head of every underlying discriminator (models/resnet3d.py; not
        # in the reference, 0 = off by default). Works with and without a sentence code, and together with proj.
        self.mbstd_on = TF.mbstd_check_group(mbstd) if mbstd != 0 else 0
        if self.mbstd_on:
            extra['mbstd'] = self.mbstd_on
        # match: the head of the contrastive clip-caption matching term (--D_match / --G_match; models/resnet3d.py; not in the
        # reference, off by default). It feeds no logit; works together with proj and mbstd. One shared trunk only.
        self.match_on = bool(match)
        if self.match_on and not self._wrap:
            raise ValueError('match (matching head) needs the text-conditioned discriminator '
                             'txt2vid.models.tganv2_cond.discrim.MultiScaleDiscrim')
        if self.match_on and cond_dim < 1:
            raise ValueError('match (matching head) needs a sentence code (cond_dim > 0): it cannot run with --dont_use_sent')
        if self.match_on and not single_discrim:
            raise ValueError('match (matching head) needs the shared trunk (single_discrim=True): one W for every pyramid level')
        if self.match_on:
            extra['match'] = True
        if single_discrim:
            d = underlying_discrim(cond_dim=cond_dim, num_down_blocks=discrim_down_blocks[-1], num_channels=num_channels, **extra)
            self.single_discrim = _ModuleWrap(d) if self._wrap else d
            self.sub_discrims = [self.single_discrim for _ in discrim_down_blocks]
        else:
            self.single_discrim = None
            subs = []
            for db in discrim_down_blocks:
                d = underlying_discrim(cond_dim=cond_dim, num_down_blocks=db, num_channels=num_channels, **extra)
                subs.append(_ModuleWrap(d) if self._wrap else d)
            self.sub_discrims = nn.ModuleList(subs)

    def refuse_proj_mismatch(self, state_dict):
        """A checkpoint written with the projection head (`*.proj.weight` keys) loads only into a discriminator built with
        proj=True, and one without into one without: a clear error instead of a bare missing / unexpected key."""
        has = any(k.endswith('proj.weight') for k in state_dict)
        if has != self.proj_on:
            raise ValueError(_PROJ_MISMATCH % ('has' if has else 'has no', self.proj_on))

    def refuse_mbstd_mismatch(self, state_dict):
        """Likewise for the minibatch standard deviation head (`*.mbstd.weight` keys) and mbstd=G."""
        has = any(k.endswith('mbstd.weight') for k in state_dict)
        if has != bool(self.mbstd_on):
            raise ValueError(_MBSTD_MISMATCH % ('has' if has else 'has no', self.mbstd_on))

    def refuse_match_mismatch(self, state_dict):
        """Likewise for the matching head (`*.match.weight` keys) and match=True."""
        has = any(k.endswith('match.weight') for k in state_dict)
        if has != self.match_on:
            raise ValueError(_MATCH_MISMATCH % ('has' if has else 'has no', self.match_on))

    def match_head(self):
        """The shared trunk's CondMatch module, or None."""
        trunk = self.single_discrim.module if isinstance(self.single_discrim, _ModuleWrap) else self.single_discrim
        return getattr(trunk, 'match', None)

    def load_state_dict(self, state_dict, strict=True, **kw):
        self.refuse_proj_mismatch(state_dict)
        self.refuse_mbstd_mismatch(state_dict)
        self.refuse_match_mismatch(state_dict)
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def forward(self, x=None, cond=None, xbar=None, computed_features=None, segs=None):
        """segs (looked at with mbstd only): per tensor of `x` the segment length of its rows for the minibatch statistic
        (default: its batch size) — the fused D step passes b for its real‖fake tensors of 2b rows."""
        if self.mbstd_on:
            return self._forward_mbstd(x, cond, xbar, segs)
        if self.single_discrim is not None and xbar is None and len(x) > 1 and x[0].is_cuda:
            trunk = self.single_discrim.module if isinstance(self.single_discrim, _ModuleWrap) else self.single_discrim
            if hasattr(trunk, 'groupable') and trunk.groupable():
                return trunk.forward_levels(list(x), None if cond is None else list(cond))
        out = []
        for i, r in enumerate(x):
            c = cond[i] if cond is not None else None
            # `computed_features` is accepted and ignored exactly like the reference (its `cf_i` is never
            # assigned, tganv2_cond/discrim.py:35,40-41), so results are identical.
            out.append(self.sub_discrims[i](r, cond=c, xbar=None if xbar is None else xbar[i]))
        return out

    def _forward_mbstd(self, x, cond, xbar, segs):
        """`forward` with the segment lengths handed on to the trunk(s)."""
        if segs is not None and len(segs) != len(x):
            raise ValueError('one segment length per tensor of x, got %d for %d' % (len(segs), len(x)))
        if self.single_discrim is not None and xbar is None and len(x) > 1 and x[0].is_cuda:
            trunk = self.single_discrim.module if isinstance(self.single_discrim, _ModuleWrap) else self.single_discrim
            if hasattr(trunk, 'groupable') and trunk.groupable():
                return trunk.forward_levels(list(x), None if cond is None else list(cond), None if segs is None else list(segs))
        return [self.sub_discrims[i](r, cond=cond[i] if cond is not None else None, xbar=None if xbar is None else xbar[i],
                                     seg=None if segs is None else segs[i]) for i, r in enumerate(x)]


class _ModuleWrap(nn.Module):
    """Stands in for the `nn.DataParallel` wrapper of the conditional discriminator so that the
    checkpoint keys stay `single_discrim.module.*`. No scatter/gather: one process = one GPU."""

    def __init__(self, module):
        super().__init__()
        self.module = module

    def forward(self, *a, **k):
        return self.module(*a, **k)
