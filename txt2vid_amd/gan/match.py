"""Contrastive clip-caption matching loss (XMC-GAN, Zhang et al. 2021; opt-in through `--D_match` / `--G_match` and
`MultiScaleDiscrim(match=True)`, not in the reference): the flags' rules, and the state the training loop carries.

The term (functional_match.py) is a symmetric InfoNCE loss between the discriminator's embedded features f W and the sentence
codes of one batch, every other caption of the batch a negative, equal captions masked. The D step adds `--D_match` times the
term of the real clips with their captions to the D loss (W = `match.weight` and the trunk learn it on real pairs); the G step
adds `--G_match` times the term of the generated clips with their captions to the G loss, through the frozen D. The term has no
state: the only checkpoint entry is W. `stats_d` / `stats_g` float32[4] = {term, clip→caption top-1 accuracy, caption→clip
top-1 accuracy, masked entries} of the last D / G step, the accuracies and the count of pyramid level 0; they travel with the
losses (gan/extras.py). τ = 0.1 and λ = 1 are XMC-GAN's values for images: nobody has tuned them for video."""
import math

import torch

N_STATS = 4


def check_args(args, world=1):
    """The rules of --D_match / --G_match / --match_tau (ValueError otherwise; NotImplementedError for --end2end). Parameter
    objects without the attributes mean "off". Data-parallel runs are allowed: the term has no state, the negatives are the
    rank's own, and W is an ordinary discriminator parameter."""
    lam_d, lam_g, tau = (getattr(args, k, None) for k in ('D_match', 'G_match', 'match_tau'))
    if lam_d is None and lam_g is None:
        if tau is not None:
            raise ValueError('--match_tau shapes --D_match / --G_match: give at least one of them')
        return args
    for flag, lam in (('--D_match', lam_d), ('--G_match', lam_g)):
        if lam is not None and not (float(lam) > 0 and math.isfinite(float(lam))):
            raise ValueError('%s takes a weight > 0 (XMC-GAN uses 1.0), got %r' % (flag, lam))
    if tau is not None and not (float(tau) > 0 and math.isfinite(float(tau))):
        raise ValueError('--match_tau takes a temperature > 0 (XMC-GAN uses 0.1), got %r' % (tau,))
    names = getattr(args, 'D_names', None) or getattr(args, 'D', None) or []
    if len(names) > 1:
        raise ValueError('--D_match / --G_match use the matching head of the first and only discriminator, %d are configured' % len(names))
    if getattr(args, 'dont_use_sent', False):
        raise ValueError('--D_match / --G_match need a sentence code: they cannot run with --dont_use_sent')
    if getattr(args, 'end2end', False):
        raise NotImplementedError('--D_match / --G_match with --end2end: the term forms no caption gradient')
    args.match_tau = 0.1 if tau is None else float(tau)
    return args


def enabled(args):
    return getattr(args, 'D_match', None) is not None or getattr(args, 'G_match', None) is not None


def head_of(discrim):
    """The CondMatch module of a discriminator, or None."""
    fn = getattr(discrim, 'match_head', None)
    return fn() if fn is not None else getattr(discrim, 'match', None)


def check_discrims(args, discrims, training=True):
    """The flags need the head (`match=True` in the --D spec), and — in a training run — the head needs the flags."""
    heads = [head_of(d) is not None for d in discrims]
    if enabled(args) and not (heads and heads[0]):
        raise ValueError('--D_match / --G_match need the matching head: pass match=True in the --D spec '
                         '(tools/cfg/discrim_cond_match.json)')
    if training and any(heads) and not enabled(args):
        raise ValueError('the --D spec builds a matching head (match=True) that nothing would train: give --D_match and / or --G_match')


class MatchState(object):
    """The term's weights and temperature and the two statistics buffers: `lam_d` / `lam_g` (None: that side is off), `tau`,
    `stats_d`, `stats_g` (device float32[4], filled by the term's launch of the last D / G step)."""

    def __init__(self, lam_d=None, lam_g=None, tau=0.1, device='cpu'):
        if lam_d is None and lam_g is None:
            raise ValueError('the matching term needs a weight for the D step, the G step or both')
        for lam in (lam_d, lam_g):
            if lam is not None and not (float(lam) > 0 and math.isfinite(float(lam))):
                raise ValueError('the weight of the term is > 0, got %r' % (lam,))
        if not (float(tau) > 0 and math.isfinite(float(tau))):
            raise ValueError('the temperature is > 0, got %r' % (tau,))
        self.lam_d = None if lam_d is None else float(lam_d)
        self.lam_g = None if lam_g is None else float(lam_g)
        self.tau = float(tau)
        self.stats_d = torch.zeros(N_STATS, dtype=torch.float32).to(device)       # (by copy: no fill kernel)
        self.stats_g = torch.zeros(N_STATS, dtype=torch.float32).to(device)
        # gan/extras.py: a side whose flag is absent has no slot and no part of the line; no checkpoint state beyond W
        self.slots = ([('match_d', self.stats_d, N_STATS)] if self.lam_d is not None else []) + \
                     ([('match_g', self.stats_g, N_STATS)] if self.lam_g is not None else [])
        self.key = None

    def term(self, head, feats, conds, side):
        """The term of one step (0-d, differentiable in the features and, in the D step, in W): `side` 'D' or 'G' picks the
        statistics buffer; in the G step D is frozen, so only the features' gradient flows."""
        if side == 'D':
            return head(list(feats), list(conds), self.tau, self.stats_d)
        return head(list(feats), list(conds), self.tau, self.stats_g, frozen=True)

    def log_lines(self, iteration, values):
        d = values.get('match_d') if self.lam_d is not None else None
        g = values.get('match_g') if self.lam_g is not None else None
        parts, masked = [], None
        if d:
            parts.append('D term %.4f, real acc %.3f / %.3f' % (d[0], d[1], d[2]))
            masked = d[3]
        if g:
            parts.append('G term %.4f, fake acc %.3f / %.3f' % (g[0], g[1], g[2]))
            masked = g[3] if masked is None else masked
        if not parts:
            return []
        return ['Iter %d, Match (tau %g): %s, masked %d' % (iteration, self.tau, ', '.join(parts), int(masked))]
