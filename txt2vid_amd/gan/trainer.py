"""Training loop of the TGANv2 hot path — same entry points and flags as txt2vid/gan/trainer.py
(`add_params_to_parser`, `train`, `test`), with the loop body factored into `train_iteration` so that
bench.py and the parity tests drive exactly what `train()` runs. `train()` meets the opt-in features that log or are read with the
losses (ada, lr schedule, gradient guard) through gan/extras.py and names none of them; the KID evaluation (`gan.kid`) is
two calls outside the step: `observe` in front of it until the real bank is full, `step` next to the sample-writing block.

Random draws follow the reference order on the HOST generators (SURVEY §7 "RNG parity"): 4x Subsample
phase (trainer.py:157-158), z (trainer.py:221, drawn on the CPU and copied), 3x Subsample in G,
gen_perm (numpy), 4x GP alpha (losses.py:140-145), gen_perm for real_pred (trainer.py:247). Under the
--discrim_steps N / --gen_steps M schedule (trainer.py:228-263): gen_perm + 4x alpha once per D step, then
gen_perm for real_pred, then 3x Subsample per later G forward (DESIGN "D:G step schedule"). With --D_aug every D step
draws a real and a generated augmentation block in front of its alphas, G part 0 a real and a generated block, every later G
step a generated block behind its forward's draws. With gated augmentation (--D_aug_p < 1 or --D_ada) every such
block is followed at once by its gate block. With a geometric name in the policy (flip, scale, rotate) every such
block is followed, behind its gate block if there is one, by its geometric block: u_real, [g_real], v_real, u_fake, [g_fake],
v_fake at a site with both lists.
"""
import argparse
import sys

import torch

from .. import functional as TF
from ..util.dir import ensure_exists
from ..util.log import status
from ..util.metrics import RollingAvg
from ..util.stopwatch import Stopwatch
from .extras import LOSSES, Readout, training_extras


def _ema_decay(text):
    v = float(text)
    if not 0.0 <= v < 1.0:
        raise argparse.ArgumentTypeError('--G_ema takes a decay in [0, 1) (0 = off), got %r' % text)
    return v


def _aug_policy(text):
    from ..functional_aug import parse_policy
    try:
        parse_policy(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError('--D_aug: %s' % e)
    return text


def _probability(text):
    v = float(text)
    if not 0.0 <= v <= 1.0:
        raise argparse.ArgumentTypeError('--D_aug_p takes a probability in [0, 1], got %r' % text)
    return v


def _ada_target(text):
    v = float(text)
    if not 0.0 < v < 1.0:
        raise argparse.ArgumentTypeError('--D_ada takes a target in (0, 1) (the paper uses 0.6), got %r' % text)
    return v


def _positive(kind, flag):
    def parse(text):
        v = kind(text)
        if not v > 0:
            raise argparse.ArgumentTypeError('%s must be positive, got %r' % (flag, text))
        return v
    return parse


def add_params_to_parser(parser):
    """Flag-for-flag txt2vid/gan/trainer.py:15-42 (including the `store_false` quirk of --no_mean_*); --no_graph, --G_ema,
    --G_ema_start, --D_aug, --D_aug_p, --D_ada, --D_ada_interval, --D_ada_kclips, --D_lecam, --D_lecam_decay, --D_lecam_start,
    --D_sn, --D_match, --G_match, --match_tau, --lr_decay, --lr_decay_iters, --lr_decay_start, --lr_final, --grad_guard, --D_clip, --G_clip, --eval_period,
    --eval_clips, --eval_block, --eval_net and --eval_prdc are new."""
    parser.add_argument('--data_is_imgs', action='store_true', default=False)
    parser.add_argument('--img_model', action='store_true', default=False)
    parser.add_argument('--log_period', type=int, default=20)
    parser.add_argument('--loss_window_size', type=int, default=20)
    parser.add_argument('--no_mean_discrim_loss', action='store_false', default=True)
    parser.add_argument('--no_mean_gen_loss', action='store_false', default=True)
    parser.add_argument('--no_graph', action='store_true', default=False, help='(new) eager launches instead of HIP-graph replay')
    parser.add_argument('--sample_batch_size', type=int, default=None)
    parser.add_argument('--discrim_steps', type=int, default=1)
    parser.add_argument('--gen_steps', type=int, default=1)
    parser.add_argument('--gp_lambda', type=float, default=-1)
    parser.add_argument('--save_initial', action='store_true', default=False)
    parser.add_argument('--save_initial_examples', action='store_true', default=False)
    parser.add_argument('--save_model_period', type=int, default=100)
    parser.add_argument('--save_example_period', type=int, default=100)
    parser.add_argument('--use_writer', action='store_true', default=False)
    parser.add_argument('--out', type=str, default='out')
    parser.add_argument('--out_samples', type=str, default='out_samples')
    parser.add_argument('--subsample_input', action='store_true', default=False)
    parser.add_argument('--G_ema', type=_ema_decay, default=0.0,
                        help='(new) decay of a moving average of the generator weights, used for samples and saved as gen_ema; 0 = off')
    parser.add_argument('--G_ema_start', type=int, default=0,
                        help='(new) the average copies the weights for the first N generator updates')
    parser.add_argument('--D_aug', type=_aug_policy, default='',
                        help='(new) differentiable augmentation of every clip the discriminator sees: a comma-separated subset of '
                             'color,translation,cutout,flip,scale,rotate; empty = off. flip, scale and rotate (x-flip with '
                             'probability 1/2, isotropic scaling by 2^(+-0.4), rotation by +-30 degrees) are one bilinear '
                             'resampling per clip, applied first; then color, translation, cutout in that order. The scaling and '
                             'rotation ranges follow the ADA paper\'s values for images: nobody has tuned them for video. Leave '
                             'flip out when captions name a side or a direction')
    parser.add_argument('--D_aug_p', type=_probability, default=None,
                        help='(new) apply each transformation of --D_aug per clip with this probability, in [0, 1]: the fixed '
                             'strength, or the initial one under --D_ada. Default 1.0 without --D_ada (every clip, as --D_aug '
                             'alone), 0.0 with it')
    parser.add_argument('--D_ada', type=_ada_target, default=None, metavar='TARGET',
                        help='(new) adaptive strength (ADA, Karras et al. 2020): steer the probability of --D_aug during training so '
                             'that the mean sign of D(real) - D(generated) over paired logits stays at TARGET, 0 < TARGET < 1 '
                             '(the paper uses 0.6). Single-GPU runs only. 0.6 and the defaults of the two flags below are the '
                             "paper's values for images: nobody has tuned them for video or for the paired statistic")
    parser.add_argument('--D_ada_interval', type=_positive(int, '--D_ada_interval'), default=4,
                        help="(new) discriminator steps per update of the probability (the paper's value for images; untuned here)")
    parser.add_argument('--D_ada_kclips', type=_positive(float, '--D_ada_kclips'), default=500.0,
                        help='(new) thousands of clips in which the probability can move from 0 to 1 '
                             "(the paper's value for images; untuned here)")
    parser.add_argument('--D_lecam', type=_positive(float, '--D_lecam'), default=None, metavar='LAMBDA',
                        help='(new) LeCam regularisation (Tseng et al. 2021): add LAMBDA > 0 times the mean squared distance of '
                             "the discriminator's unconditional logits on real / generated clips to a moving average of its "
                             'logits on generated / real clips. One discriminator, single-GPU runs only. The paper uses 0.3 with '
                             'hinge-scale logits on images: nobody has tuned it for video or for the relativistic loss')
    parser.add_argument('--D_lecam_decay', type=float, default=None, metavar='DECAY',
                        help='(new) decay of the moving averages of --D_lecam, in [0, 1) (default 0.99)')
    parser.add_argument('--D_lecam_start', type=int, default=None, metavar='N',
                        help='(new) discriminator steps before the term of --D_lecam counts; the averages move from the first '
                             'step (default 0)')
    parser.add_argument('--D_sn', action='store_true', default=False,
                        help='(new) spectral normalisation of every Conv3d / Linear weight of the discriminators: one power '
                             'iteration after each discriminator update')
    parser.add_argument('--D_match', type=_positive(float, '--D_match'), default=None, metavar='LAMBDA',
                        help='(new) contrastive clip-caption matching (XMC-GAN, Zhang et al. 2021): add LAMBDA > 0 times a symmetric '
                             "InfoNCE loss between the discriminator's embedded features of the real clips and their sentence "
                             'codes to the D loss; every other caption of the batch is a negative, equal captions are masked. '
                             'Needs match=True in the --D spec (tools/cfg/discrim_cond_match.json); one discriminator, not with '
                             "--end2end. XMC-GAN uses 1.0 on images: nobody has tuned it for video")
    parser.add_argument('--G_match', type=_positive(float, '--G_match'), default=None, metavar='LAMBDA',
                        help='(new) add LAMBDA > 0 times the same loss of the generated clips with their captions, through the '
                             'frozen discriminator, to the G loss (same requirements as --D_match; either or both). Alone, nothing trains '
                             'the head: G is then trained against its fixed initial random projection, or a loaded one')
    parser.add_argument('--match_tau', type=float, default=None, metavar='TAU',
                        help="(new) temperature of --D_match / --G_match (default 0.1, XMC-GAN's value for images; untuned here)")
    parser.add_argument('--lr_decay', choices=('none', 'linear', 'cosine'), default='none',
                        help='(new) decay --G_lr and --D_lr by one factor per training iteration, inside the replayed graph: '
                             'linear or cosine from 1 at --lr_decay_start to --lr_final at --lr_decay_iters. '
                             '--lr_decay linear --lr_decay_iters 100000 is the TGANv2 recipe')
    parser.add_argument('--lr_decay_iters', type=int, default=None, metavar='T',
                        help='(new) the training iteration at which the decay ends (required with --lr_decay); the rate stays at '
                             'its final value from there on')
    parser.add_argument('--lr_decay_start', type=int, default=None, metavar='S',
                        help='(new) iterations at the full rate before the decay begins (default 0)')
    parser.add_argument('--lr_final', type=float, default=None, metavar='F',
                        help='(new) the fraction of the base rate that remains at the end, in [0, 1] (default 0)')
    parser.add_argument('--grad_guard', action='store_true', default=False,
                        help='(new) measure the global gradient norm in front of both optimiser steps, inside the replayed graph, '
                             'and skip a step whose norm is inf or NaN (parameters, moments and step count stay as they are)')
    parser.add_argument('--D_clip', type=float, default=None, metavar='C',
                        help="(new) clip the discriminator's gradients to global L2 norm C > 0 "
                             '(torch.nn.utils.clip_grad_norm_ semantics); implies --grad_guard')
    parser.add_argument('--G_clip', type=float, default=None, metavar='C',
                        help="(new) clip the generator's gradients to global L2 norm C > 0; implies --grad_guard")
    from .kid import add_flags as add_kid_flags
    add_kid_flags(parser)                  # --eval_period, --eval_clips, --eval_block, --eval_net, --eval_prdc (new)
    return parser


def multiscale_data(x, cond, frame_sizes, subsample_input=True):
    """Real-data pyramid — trainer.py:131-165. x: [B,C,T,H,W] on the device. Level i is the nearest
    resize of the (progressively batch/time sub-sampled) clip to frame_sizes[i]; one gather kernel per
    level does sub-sampling and resize in a single pass over the source. The Subsample phases come from
    `TF.draws` (host generator; device-resident under graph replay)."""
    n = len(frame_sizes)
    if n == 1:
        return [x], (None if cond is None else [cond])
    B, Cc, T, H, W = x.shape
    if subsample_input:
        t0s = TF.draws.multiscale_t0(n)
    else:
        t0s = [(0, None)] * n
    xs, conds = [], []
    sb, st = 1, 1                  # level tensor == x[::sb, :, t0::st]
    Bl, Tl = B, T
    for i in range(n):
        fs = frame_sizes[i] if i != n - 1 else None
        Ho, Wo = (fs, fs) if fs is not None else (H, W)
        t0, t0_dev = t0s[i]
        if sb == 1 and st == 1 and Ho == H and Wo == W:
            xs.append(x)
        else:
            xs.append(TF.pyramid_gather(x, Bl, Tl, Ho, Wo, sb, st, t0, t0_dev))
        if cond is not None:
            conds.append(cond)
        if subsample_input:
            if Tl % 2:
                raise ValueError('subsample_input needs a frame count divisible by 2**levels')
            st, sb = st * 2, sb * 2
            Bl, Tl = (Bl + 1) // 2, Tl // 2
            if cond is not None:
                # cond[::2] (trainer.py:160); --end2end keeps the sentence code's graph, so the slice must be differentiable
                cond = cond[::2] if cond.requires_grad else TF.stride_rows(cond, 2)
    return xs, (conds if conds else None)


class TrainStep(object):
    """The loop body trainer.py:199-267 after data loading, for the schedule of N = --discrim_steps D steps and
    M = --gen_steps G steps, cut after every backward pass (where data-parallel ranks exchange gradients):
      D part 0   pyramid, G forward, D loss + GP, D backward                     |sync D grads|
      D part j   Adam on D, D loss + GP, D backward                  (1 <= j < N) |sync D grads|
      G part 0   Adam on D, real_pred / fused G loss, G backward                  |sync G grads|
      G part j   Adam on G, G re-forward (same z), G loss, G backward (1 <= j < M) |sync G grads|
      end        Adam on G.
    N = M = 1 is the three parts part_d | part_g | part_end. Eager mode runs the parts back to back;
    `GraphedTrainStep` captures them as HIP graphs."""

    def __init__(self, gan, optD, optG, losses, params, device, end2end=False, grad_sync=None):
        self.n_d, self.n_g = int(params.discrim_steps), int(params.gen_steps)
        if self.n_d < 1 or self.n_g < 1:
            raise ValueError('--discrim_steps and --gen_steps must be >= 1 (got %d and %d)' % (self.n_d, self.n_g))
        self.gan, self.optD, self.optG, self.losses, self.params = gan, optD, optG, losses, params
        self.device, self.end2end, self.grad_sync = device, end2end, grad_sync
        self.lD = self.lG = self.fake = self.xs = self.conds = None
        self._z = self._real_pred = None
        # conditioning augmentation of the generator (MultiScaleGen(ca_dim > 0), not in the reference): every G step's loss gains
        # ca_kl_coeff * KL of that step's forward; lKL totals the KL over the G steps like lG (device-side)
        gen = getattr(gan, 'gen', None)
        self.ca = bool(getattr(gen, 'ca_dim', 0))
        self.kl_coeff = float(getattr(gen, 'ca_kl_coeff', 0.0)) if self.ca else 0.0
        self.lKL = self._kl = None
        # differentiable augmentation of D's inputs (--D_aug, not in the reference; functional_aug): every list of clips handed to
        # discrim_step / gen_step / gen_step_fused / the real_pred pass goes through ONE grouped launch first (real + generated),
        # with fresh parameter blocks per D step and per G step. Parameter objects without the attribute mean "off".
        from ..functional_aug import GEO, parse_policy
        self.aug = parse_policy(getattr(params, 'D_aug', ''))
        self.geo = self.aug & GEO         # flip / scale / rotate: their own launch in front, one more block per site
        self._xs_g = None                 # the augmented real pyramid of G part 0 (reused by later fused G steps)
        # adaptive strength (--D_aug_p / --D_ada): each transformation applied per clip with probability p, read from
        # device memory by the gated launches. p is the controller's (gan.ada, updated behind every D forward) or a fixed value;
        # --D_aug_p 1.0 without a controller is the ungated path: no gate draws, the old entry points
        from .ada import check_args
        check_args(params)
        self.ada = getattr(gan, 'ada', None) if self.aug else None
        if getattr(gan, 'ada', None) is not None and not self.aug:
            raise ValueError('a controller of the augmentation strength (gan.ada) needs a non-empty --D_aug')
        if self.ada is not None and grad_sync is not None:
            raise ValueError('--D_ada in a data-parallel run: synchronising the window across ranks is not implemented')
        p_fixed = getattr(params, 'D_aug_p', None)
        self.gated = bool(self.aug) and (self.ada is not None or (p_fixed is not None and p_fixed != 1.0))
        self._p = None
        if self.gated:
            self._p = self.ada.p if self.ada is not None else _fixed_p(p_fixed, device)
        # learning-rate decay (--lr_decay): the optimisers tick and read device-resident schedule states themselves; the
        # only thing to hold here is that the states count this schedule's steps per iteration
        for opt, n, flag in ((optD, self.n_d, '--discrim_steps'), (optG, self.n_g, '--gen_steps')):
            sch = getattr(opt, 'lr_sched', None)
            if sch is not None and sch.spi != n:
                raise ValueError('the learning-rate schedule counts %d optimiser steps per iteration, %s is %d' % (sch.spi, flag, n))
        # the clip-caption matching term (--D_match / --G_match) forms no caption gradient
        if getattr(gan, 'match', None) is not None and end2end:
            raise NotImplementedError('--D_match / --G_match with --end2end: the term forms no caption gradient')
        self._fused = False
        self._one = None                  # dL/dL = 1 for both backward passes: one persistent 0-d tensor (no fill launch per pass)
        # the store_false quirk of --no_mean_*_loss (trainer.py:236-237,260-261): the loss of every step is divided by the step
        # count only when the flag was PASSED (its value is then False)
        self.d_scale = 1.0 if getattr(params, 'no_mean_discrim_loss', True) else 1.0 / self.n_d
        self.g_scale = 1.0 if getattr(params, 'no_mean_gen_loss', True) else 1.0 / self.n_g
        # the backward roots 1/N, 1/M: filled here, outside any graph capture, and never written again
        self._scaled = {}
        if torch.device(device).type == 'cuda':
            for s in {self.d_scale, self.g_scale} - {1.0}:
                self._scaled[s] = TF.full_scalar(s, device)
        # weight / bias gradients land directly in flat per-model arenas (the ones the data-parallel exchange
        # all-reduces, when there is one): no per-parameter sums, no gather copies
        self.grad_sink = None
        if not end2end and torch.device(device).type == 'cuda':
            cached = gan.__dict__.get('_t2v_grad_sink')
            if cached is None or cached[0] is not grad_sync:
                from ..dist import model_arena
                arenas = list(grad_sync.arenas.values()) if grad_sync is not None else [
                    model_arena(list(gan.discrims), TF.copy_into), model_arena(gan.gen, TF.copy_into)]
                cached = (grad_sync, TF.GradSink(arenas))
                gan.__dict__['_t2v_grad_sink'] = cached          # one pair of arenas per model, reused by every step
            self.grad_sink = cached[1]

    def _root(self, loss, scale=1.0):
        if scale != 1.0:
            return self._scaled[scale].view(loss.shape)
        if self._one is None or self._one.device != loss.device or self._one.shape != loss.shape:
            self._one = TF.ones_like(loss.detach())
        return self._one

    def _arm_sink(self):
        TF.set_grad_sink(self.grad_sink)
        TF.grad_sink_reset()              # the step about to run clears this model's gradients first

    @staticmethod
    def _total(total, loss, scale):
        """total + scale * loss on the device (the reference's `total_*_loss += float(loss)`, without a host sync)."""
        loss = loss.detach()
        if total is None:
            return loss if scale == 1.0 else TF.scalar_sum([loss], weights=[scale])
        return TF.scalar_sum([total, loss], weights=[1.0, scale])

    def _forward_g(self):
        cond = self.conds[0] if self.conds is not None else None
        if self.ca:
            fake, self._kl = self.gan(self._z, cond=cond, return_kl=True)      # CA draws this forward's eps before its phases
            return fake
        return self.gan(self._z, cond=cond)

    def _augment(self, real, fake):
        """(real, fake) through the augmentation, both lists (either may be None) in one launch: a block of draws for the real
        clips first, then one for the generated clips. Under --subsample_input level l's sample j reads base row j * 2^l. Gated:
        every block comes with its gate block, and the launch reads the current p. With a geometric name in the policy every
        block also comes with its geometric block v, and the clips go through the resampling launch first (geometry, then colour,
        translation, cutout)."""
        if not self.aug:
            return real, fake
        from ..functional_aug import diffaug, geoaug
        xs, us, gs, vs, strides = [], [], [], [], []
        for clips in (real, fake):
            if clips is None:
                continue
            g = v = None
            if self.geo:
                got = TF.draws.aug(self._batch, self.device, gated=self.gated, geo=True)    # u, [g], v: one after the other
                u, v = got[0], got[-1]
                if self.gated:
                    g = got[1]
            elif self.gated:
                u, g = TF.draws.aug(self._batch, self.device, gated=True)         # the gate block right behind its parameter block
            else:
                u = TF.draws.aug(self._batch, self.device)
            for l, t in enumerate(clips):
                xs.append(t)
                us.append(u)
                gs.append(g)
                vs.append(v)
                strides.append(2 ** l if self.params.subsample_input else 1)
        if self.geo:
            xs = geoaug(xs, vs, strides, self.geo, gs, self._p) if self.gated else geoaug(xs, vs, strides, self.geo)
        out = diffaug(xs, us, strides, self.aug, gs, self._p) if self.gated else diffaug(xs, us, strides, self.aug)
        n = len(real) if real is not None else 0
        return (out[:n] if real is not None else None), (out[n:] if fake is not None else None)

    def _d_step(self, arm=True):
        p = self.params
        if arm:
            self._arm_sink()
        real, fake = self._augment(self.xs, [f.detach() for f in self.fake])
        loss = self.gan.discrim_step(real=real, fake=fake, cond=self.conds,
                                     loss=self.losses.discrim_loss, gp_lambda=p.gp_lambda)
        loss.backward(gradient=self._root(loss, self.d_scale), retain_graph=self.end2end)
        TF.grad_sink_flush()              # the weight-gradient partial sums of the whole pass, summed in one launch
        self.lD = self._total(self.lD, loss, self.d_scale)

    def part_d(self, x, cond):
        """D part 0: pyramid, z, G forward and the first D step."""
        p = self.params
        self.lD = self.lG = self._real_pred = self.lKL = self._xs_g = None
        self._batch = x.size(0)
        self._arm_sink()
        self.xs, self.conds = multiscale_data(x, cond, p.frame_sizes, p.subsample_input)
        self._z = TF.draws.z(x.size(0), self.gan.gen.latent_size, self.device)       # CPU generator, then copy (parity)
        self.fake = self._forward_g()
        self._d_step(arm=False)

    def part_d_more(self):
        """D part j >= 1: D's update from step j - 1, then D step j against the same pyramid and the same generated clips."""
        self.optD.step()
        self._d_step()

    def part_g(self):
        """G part 0: D's last update, real_pred (ONE pass per iteration, trainer.py:247) and the first G step."""
        self.optD.step()
        self._arm_sink()
        # D after its update, on the real batch (trainer.py:247). Its graph is only needed when the text
        # encoder trains end-to-end; otherwise nothing upstream of these predictions receives a gradient
        # that is ever used, so none is recorded (identical results, SURVEY §7 "wasted work").
        xs, fake = self._augment(self.xs, self.fake)
        self._fused = not self.end2end and self.gan.can_fuse_gen_step(fake, xs)
        if self._fused:
            if self.n_g > 1:
                self._xs_g = xs
            loss = self.gan.gen_step_fused(fake=fake, real=xs, cond=self.conds, loss=self.losses.gen_loss, **self._kl_args())
        else:
            if self.end2end:
                _, _, real_pred = self.gan.all_discrim_forward(real=xs, cond=self.conds, fake=None, loss=None)
            else:
                with torch.no_grad():
                    _, _, real_pred = self.gan.all_discrim_forward(real=xs, cond=self.conds, fake=None, loss=None)
            if self.n_g > 1:
                self._real_pred = real_pred
            loss = self.gan.gen_step(fake=fake, real_pred=real_pred, cond=self.conds, loss=self.losses.gen_loss,
                                     **self._kl_args())
        self._g_backward(loss, last=self.n_g == 1)

    def part_g_more(self, last):
        """G part j >= 1: G's update from step j - 1, a new train-mode G forward of the same z (new Subsample phases, BatchNorm
        buffers updated again) and G step j against the same real_pred. D is unchanged since G part 0, so the fused pass
        recomputes the same real_pred; it draws no caption permutation (the reference draws that one once, trainer.py:247)."""
        self._g_update()
        self._arm_sink()
        self.fake = self._forward_g()
        _, fake = self._augment(None, self.fake)          # (the real clips keep G part 0's transformation)
        if self._fused:
            loss = self.gan.gen_step_fused(fake=fake, real=self._xs_g, cond=self.conds, loss=self.losses.gen_loss,
                                           draw_perm=False, **self._kl_args())
        else:
            loss = self.gan.gen_step(fake=fake, real_pred=self._real_pred, cond=self.conds, loss=self.losses.gen_loss,
                                     **self._kl_args())
        self._g_backward(loss, last)

    def _kl_args(self):
        return {'kl': self._kl, 'kl_coeff': self.kl_coeff} if self.ca else {}

    def _g_backward(self, loss, last):
        # --end2end: real_pred and the sentence code keep their graphs for the next G step (trainer.py:262)
        loss.backward(gradient=self._root(loss, self.g_scale), retain_graph=self.end2end and not last)
        TF.grad_sink_flush()
        self.lG = self._total(self.lG, loss, self.g_scale)
        if self.ca:
            self.lKL = self._total(self.lKL, self._kl, self.g_scale)
            self._kl = None
        if last:
            self._real_pred = self._xs_g = None

    def _g_update(self):
        """G's optimiser step and, when the generator's weights are averaged (--G_ema), the average's update right behind it
        (one tick + one launch per 64 tensors, inside whatever captures this part; nothing without an average)."""
        self.optG.step()
        ema = getattr(self.gan, 'gen_ema', None)
        if ema is not None:
            ema.update()

    def part_end(self):
        self._g_update()

    @property
    def n_parts(self):
        return self.n_d + self.n_g + 1

    def part(self, k, x=None, cond=None):
        """Run part k of `n_parts`. Returns which model's gradients the data-parallel ranks exchange after it ('D', 'G', or None
        after the last part)."""
        N, M = self.n_d, self.n_g
        if k == 0:
            self.part_d(x, cond)
        elif k < N:
            self.part_d_more()
        elif k == N:
            self.part_g()
        elif k < N + M:
            self.part_g_more(last=k == N + M - 1)
        else:
            self.part_end()
            return None
        return 'D' if k < N else 'G'

    def run(self, x, cond=None):
        for k in range(self.n_parts):
            which = self.part(k, x, cond)
            if which is not None and self.grad_sync is not None:
                self.grad_sync(which)
        return self.lD, self.lG, self.fake, self.xs


_FIXED_P = {}


def _fixed_p(p, device):
    """A fixed probability as one float in device memory (made once per value and device, by copy: no fill launch per step)."""
    key = (str(torch.device(device)), float(p))
    if key not in _FIXED_P:
        _FIXED_P[key] = torch.tensor([float(p)], dtype=torch.float32).to(device)
    return _FIXED_P[key]


def train_iteration(gan, x, cond, optD, optG, losses, params, device, end2end=False, z=None, grad_sync=None):
    """One eager pass of the loop body. x: [B,C,T,H,W] device tensor. Returns (lossD, lossG, fake, xs);
    the losses are 0-d device tensors (no host sync here)."""
    return TrainStep(gan, optD, optG, losses, params, device, end2end, grad_sync).run(x, cond)


class GraphedTrainStep(object):
    """HIP-graph replay of the training iteration: after `warmup` eager iterations the N + M + 1 parts of `TrainStep`
    are captured once (shared memory pool) and every later iteration is N + M + 1 graph launches + the N + M eager
    gradient exchanges between them (one process: ONE graph for the whole iteration). All per-iteration randomness is drawn
    on the host in the reference's order and uploaded into fixed buffers before the replay
    (`functional.StaticDraws`); the batch is copied into a fixed input buffer."""

    def __init__(self, gan, optD, optG, losses, params, device, batch_shape, grad_sync=None, warmup=3, cond_dim=0):
        self.ts = TrainStep(gan, optD, optG, losses, params, device, False, grad_sync)
        self.device, self.grad_sync, self.warmup = device, grad_sync, warmup
        n_levels = len(params.frame_sizes)
        N, M = self.ts.n_d, self.ts.n_g
        self.draws = TF.StaticDraws(device, batch_shape[0], gan.gen.latent_size, n_levels, n_gen_phases=n_levels - 1,
                                    gp=params.gp_lambda > 0, subsample_input=params.subsample_input,
                                    n_perms=(N + 1) * len(gan.discrims) if cond_dim else 0, n_d_steps=N, n_g_steps=M,
                                    ca_dim=getattr(gan.gen, 'ca_dim', 0) if cond_dim else 0,
                                    n_aug=(2 * N + M + 1) * (2 if self.ts.gated else 1) if self.ts.aug else 0,
                                    n_geo=2 * N + M + 1 if self.ts.geo else 0)
        self.x = torch.empty(batch_shape, device=device, dtype=torch.float32)
        # conditional path: the sentence code is computed outside the graphs (its sequence length varies) into a fixed buffer
        self.cond = torch.empty((batch_shape[0], cond_dim), device=device, dtype=torch.float32) if cond_dim else None
        self.graphs = None
        self.n_graphs = 0                    # graphs per iteration of the last capture (1 without a gradient exchange, else N + M + 1)
        self.exchanges = ()                  # the gradient exchanges between them ('D' x N, 'G' x M)
        self.n = 0
        # warm-up and capture run on ONE side stream (the autograd graph's AccumulateGrad nodes remember
        # the stream they were created on; capture must see the same one)
        self.side = torch.cuda.Stream(device=device)

    def _eager(self):
        self.ts.run(self.x, self.cond)

    def _capture(self):
        for opt in (self.ts.optD, self.ts.optG):
            opt.make_capturable(self.device)
        # drop every reference into the previous iteration's autograd graph before capturing
        self.ts.lD = self.ts.lG = self.ts.fake = self.ts.xs = self.ts.conds = self.ts._real_pred = None
        self.ts.lKL = self.ts._kl = self.ts._xs_g = None
        torch.cuda.synchronize()
        self.draws.rewind()
        gs = self.grad_sync
        # thread-local capture mode: the data loader's pin-memory thread keeps issuing pinned allocations and H2D copies
        # while this thread captures; in the default (global) mode any such call invalidates the capture
        mode = 'thread_local'
        n_parts = self.ts.n_parts
        if gs is None:
            # one process, no gradient exchange between the parts: the whole iteration is ONE graph (fewer replay launches)
            g1 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g1, stream=self.side, capture_error_mode=mode):
                for k in range(n_parts):
                    self.ts.part(k, self.x, self.cond)
            torch.cuda.synchronize()
            self.graphs = (g1,)
            self.n_graphs = 1
            self.exchanges = ()
            if self.ts.grad_sink is not None:
                self.ts.grad_sink.frozen += 1
            return
        # data-parallel: one graph per part (shared memory pool); the exchange of the gradients the part computed sits after it
        graphs, exchanges = [], []
        for k in range(n_parts):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=graphs[0].pool() if graphs else None, stream=self.side, capture_error_mode=mode):
                which = self.ts.part(k, self.x, self.cond)
                if which is not None:
                    gs.pre(which)           # p.grad -> arena: captured (the replayed backward rewrites the same buffers)
            graphs.append(g)
            if which is not None:
                exchanges.append(which)
                gs.exchange(which)
                gs.post(which)              # Adam (captured next) reads the arena views
        torch.cuda.synchronize()
        self.graphs = tuple(graphs)
        self.n_graphs = len(graphs)
        self.exchanges = tuple(exchanges)
        if self.ts.grad_sink is not None:
            self.ts.grad_sink.frozen += 1        # the graphs bake in the sink's slab addresses and table slots

    def release(self):
        """Drop the captured graphs (a new batch shape is about to be captured): the gradient sink may grow / recycle again."""
        if self.graphs is not None:
            torch.cuda.synchronize()
            self.graphs = None
            if self.ts.grad_sink is not None:
                self.ts.grad_sink.frozen = max(0, self.ts.grad_sink.frozen - 1)

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def step(self, x, cond=None):
        """x: [B,C,T,H,W] device (or pinned host) tensor; cond: [B,cond_dim] sentence codes (conditional path). Returns
        (lossD, lossG) 0-d device tensors that are overwritten by the next call."""
        old = TF.draws
        TF.set_draws(self.draws)
        try:
            self.draws.begin_step()                      # (host RNG work first: the launches below then reach the queue back to back)
            if x.is_cuda and x.dtype == torch.float32 and x.shape == self.x.shape:
                TF.copy_into(x, self.x)                  # (a copy kernel: stays on the compute queue in front of the graph, see StaticDraws.begin_step)
            else:
                self.x.copy_(x, non_blocking=True)
            if self.cond is not None:
                TF.copy_into(cond.detach(), self.cond)
            if self.graphs is None and self.n >= self.warmup:
                self._capture()          # the capture pass also executes nothing: replay right after
            if self.graphs is None:
                cur = torch.cuda.current_stream(self.device)
                self.side.wait_stream(cur)
                with torch.cuda.stream(self.side):
                    self._eager()
                cur.wait_stream(self.side)
            else:
                self.graphs[0].replay()
                # data-parallel: the N + M exchanges sit between the N + M + 1 captured parts
                for which, g in zip(self.exchanges, self.graphs[1:]):
                    if self.grad_sync is not None:
                        self.grad_sync.exchange(which)
                    g.replay()
            self.n += 1
        finally:
            TF.set_draws(old)
        return self.ts.lD, self.ts.lG


class GraphedSentenceEncoder(object):
    """HIP-graph replay of the sentence encoder's forward (`cond_encoder.encode`, ~90 small launches: embedding gather, one GEMM
    per layer and direction, one launch per time step): one graph per sequence length — caption batches differ in their longest
    caption, and the per-sample lengths are read on the device. The first batch of a new length runs eagerly (it also fills the
    packed / transposed weight caches), the second is captured, later ones replay. Returns the sentence codes [B, encoding] in a
    buffer that the next call of the same length overwrites."""

    def __init__(self, cond_encoder, device):
        self.enc, self.device = cond_encoder, device
        self.entries = {}                # (B, L) -> [tokens int32 [B,L], lengths int32 [B], graph | None, codes | None, last lengths]
        self.side = torch.cuda.Stream(device=device)
        self.ring = [torch.zeros((1024,), dtype=torch.int32).pin_memory() for _ in range(8)]
        self.ring_pos = 0

    def encode(self, tokens, lengths):
        B, L = int(tokens.shape[0]), int(lengths[0])
        if B > 1024:
            return self.enc.encode(tokens, lengths)[2].detach()
        ent = self.entries.get((B, L))
        if ent is None:
            ent = [torch.zeros((B, L), dtype=torch.int32).to(self.device), torch.zeros((B,), dtype=torch.int32).to(self.device),
                   None, None]
            self.entries[(B, L)] = ent
            return self.enc.encode(tokens, lengths)[2].detach()
        tok, len_dev, graph, codes = ent[:4]
        tok.copy_(tokens[:, :L], non_blocking=True)                         # int64 -> int32, device or (pinned) host source
        lens = [int(n) for n in lengths]
        if len(ent) < 5 or ent[4] != lens:
            # upload through a small ring of pinned buffers: a pageable source would make the host wait for the stream (and
            # with it for the previous iteration) before it can go on to launch this one
            slot = self.ring[self.ring_pos % len(self.ring)]
            self.ring_pos += 1
            slot[:B].copy_(torch.tensor(lens, dtype=torch.int32))
            len_dev.copy_(slot[:B], non_blocking=True)
            if len(ent) < 5:
                ent.append(lens)
            else:
                ent[4] = lens
        if graph is None:
            graph = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=self.side, capture_error_mode='thread_local'):
                codes = self.enc.encode(tok, (L, len_dev))[2]
            ent[2], ent[3] = graph, codes
        graph.replay()
        return codes


def test(gan=None, num_samples=1, dataset=None, device=None, params=None, channel_first=True, vocab=None):
    """Sampling path — trainer.py:44-90. `num_samples` times: take the FIRST batch of the loader (the reference `break`s after
    one), encode its captions, draw z, run the eval-mode generator (one full [B,C,16,S,S] clip per latent: no sub-sampling,
    last level only unless `output_blocks` asks for more) and write, with the reference's file names,
    `real_<i>.png`, `sentences_<i>_<j>.txt` and one `<h>x<w>_<i>_<j>.jpg` grid per rendered level."""
    from .samples import save_frames, save_sentences
    from ..data import DevicePrefetcher
    ensure_exists(params.out_samples)
    gan.gen.eval()
    with torch.no_grad():
        for i in range(num_samples):
            pre = DevicePrefetcher(dataset, device)
            j = 0
            x, y = pre.next()
            if x is None:
                break
            x = TF.video_to_channel_first(x)
            cond = None
            if gan.cond_encoder is not None and len(y) >= 2:
                _, _, cond = gan.cond_encoder.encode(y[0], y[1])
            z = torch.randn(x.size(0), gan.gen.latent_size).to(device)
            ema = getattr(gan, 'gen_ema', None)
            if ema is not None:
                status('sampling from the averaged generator (%d updates)' % ema.updates)
                with ema.swapped():
                    fake = gan(z, cond=cond)
            else:
                fake = gan(z, cond=cond)
            save_frames(x, '%s/real_%d.png' % (params.out_samples, i), is_images=getattr(params, 'img_model', False))
            if cond is not None and vocab is not None:
                save_sentences(y[0], path='%s/sentences_%d_%d.txt' % (params.out_samples, i, j), vocab=vocab)
            for f in fake:
                h, w = f.size(3), f.size(4)
                path = '%s/%dx%d_%d_%d.jpg' % (params.out_samples, h, w, i, j)
                status('saving to %s' % path)
                save_frames(f, path, is_images=getattr(params, 'img_model', False))
    gan.gen.train()


def _averaged_samples(gan, z, cond):
    """The iteration's z (and sentence codes) through the AVERAGED generator, every level rendered: one extra eval-mode forward
    outside the captured graph (a train-mode one would update the BatchNorm buffers a second time), only on iterations that
    write a grid. Eval mode renders full clips at every level (no sub-sampling)."""
    gen = gan.gen
    was_training = gen.training
    gen.eval()
    try:
        with torch.no_grad(), gan.gen_ema.swapped():
            return gan(z.detach(), cond=None if cond is None else cond.detach(), output_blocks=range(len(gen.render_blocks)))
    finally:
        gen.train(was_training)


def train(gan=None, num_epoch=None, dataset=None, device=None, optD=None, optG=None, params=None, vocab=None, losses=None,
          channel_first=True, end2end=True, grad_sync=None, max_iters=None):
    """txt2vid/gan/trainer.py:111-333. `dataset` yields (videos [B,T,C,H,W], tokens, lengths) batches
    (host tensors); a pinned-memory prefetch thread overlaps H2D with the step."""
    assert channel_first
    if params.sample_batch_size is None:
        params.sample_batch_size = params.batch_size
    ensure_exists(params.out)
    ensure_exists(params.out_samples)
    avg = {name: RollingAvg(window_size=params.loss_window_size) for name in LOSSES}     # (kl: conditioning augmentation only)
    # the opt-in features that log or travel with the losses (gan/extras.py), and the host values last read for them
    extras, seen = training_extras(gan, optD, optG), {}
    avg_iter = RollingAvg(window_size=max(1, params.log_period))
    avg_load = RollingAvg(window_size=max(1, params.log_period))
    load_watch, iter_watch = Stopwatch(), Stopwatch()
    from ..data import DevicePrefetcher
    from ..dist import rank_world
    writer = rank_world()[0] == 0            # data-parallel replicas are identical: rank 0 alone writes checkpoints and samples
    kid = getattr(gan, 'kid', None) if writer else None      # --eval_period: the writer alone, from its local batches
    iteration = 0
    # HIP-graph replay of the iteration (see GraphedTrainStep) unless --no_graph / --end2end: the eager loop is
    # host-bound (~1 000 launches at ~20 us of Python each)
    use_graph = not end2end and not getattr(params, 'no_graph', False) and torch.device(device).type == 'cuda'
    graphed, graphed_key, graphed_encoder = None, None, None
    readout = Readout(extras, device) if use_graph else None
    for epoch in range(num_epoch):
        if params.log_period > 0:
            status('Epoch %d started' % (epoch + 1))
        load_watch.start()
        iter_watch.start()
        if hasattr(getattr(dataset, 'sampler', None), 'set_epoch'):
            dataset.sampler.set_epoch(epoch)                 # a new permutation per epoch on every rank
        pre = DevicePrefetcher(dataset, device)
        i = 0
        x, y = pre.next()
        while x is not None:
            iteration = epoch * len(dataset) + i + 1
            load_watch.stop()
            avg_load.update(load_watch.elapsed_time)
            x = TF.video_to_channel_first(x)                      # [B,T,C,H,W] -> [B,C,T,H,W] (trainer.py:204)
            cond = None
            if gan.cond_encoder is not None and len(y) >= 2:
                if use_graph:
                    if graphed_encoder is None:
                        graphed_encoder = GraphedSentenceEncoder(gan.cond_encoder, device)
                    cond = graphed_encoder.encode(y[0], y[1])
                else:
                    _, _, cond = gan.cond_encoder.encode(y[0], y[1])
                    if not end2end:
                        cond = cond.detach()
            if kid is not None and not kid.full:
                kid.observe(x, cond)             # the first clips of the run fill the real bank (eager launches, between replays)
            if use_graph:
                key = (tuple(x.shape), None if cond is None else tuple(cond.shape))
                if graphed is None or key != graphed_key:          # first batch (or a new batch shape): capture again
                    if graphed is not None:
                        graphed.release()
                    graphed = GraphedTrainStep(gan, optD, optG, losses, params, device, tuple(x.shape), grad_sync=grad_sync,
                                               warmup=2, cond_dim=0 if cond is None else cond.shape[1])
                    graphed_key = key
                    if params.log_period > 0:
                        status('HIP-graph replay of the iteration for batches of shape %s (2 eager iterations, then capture)' % (key[0],))
                lD, lG = graphed.step(x, cond)
                fake, xs = graphed.ts.fake, graphed.ts.xs
                # the losses and the extras' floats are read ONE iteration late (Readout): the rolling averages lag by one
                readout.push(iteration, lD=lD, lG=lG, kl=graphed.ts.lKL)
                got = readout.pop() or {}
            else:
                ts = TrainStep(gan, optD, optG, losses, params, device, end2end, grad_sync)       # (= train_iteration)
                lD, lG, fake, xs = ts.run(x, cond)
                got = {name: [float(t)] for name, t in zip(LOSSES, (lD, lG, ts.lKL)) if t is not None}
                if params.log_period > 0 and iteration % params.log_period == 0:         # the extras' slots, read on the spot
                    got.update({name: t[:n].tolist() for e in extras for name, t, n in e.slots})
            for name in LOSSES:
                if name in got:
                    avg[name].update(got.pop(name)[0])
            seen.update(got)
            # checkpoint: the reference tests `save_example_period` here (trainer.py:269) and never reads
            # --save_model_period; the intended flag is used (SURVEY §8a defect 3).
            if writer and ((iteration == 1 and params.save_initial) or (params.save_model_period > 0 and
                                                                        iteration % params.save_model_period == 0)):
                from ..train.setup import get_rng_state
                # extra keys next to the reference's layout (its loader ignores them; its files, which lack them, still load here)
                to_save = {'optG': optG.state_dict(), 'optD': optD.state_dict(), 'iteration': iteration, 'rng_state': get_rng_state()}
                to_save.update(gan.save_dict())          # (with the keys of the extras the models own)
                to_save.update({e.key: e.state_dict() for e in extras if e.key})
                torch.save(to_save, '%s/iter_%d_lossG_%.4f_lossD_%.4f' % (params.out, iteration, avg['lG'].get(), avg['lD'].get()))
            if params.log_period > 0 and iteration % params.log_period == 0:
                sys.stdout.flush()
                status('[%d/%d; %d/%d] - Iter %d, Loss_D: %.4f Loss_G: %.4f (%.2fGB used; %.2fGB cached) - %.4f sec/iter; '
                       '%.4f sec/batch load' % (epoch, num_epoch, i, len(dataset), iteration, avg['lD'].get(),
                                                avg['lG'].get(), torch.cuda.max_memory_allocated() / 1e9,
                                                torch.cuda.max_memory_reserved() / 1e9, avg_iter.get(), avg_load.get()))
                if getattr(gan.gen, 'ca_dim', 0):
                    status('Iter %d, KL (conditioning augmentation, inside Loss_G with weight %g): %.4f' %
                           (iteration, gan.gen.ca_kl_coeff, avg['kl'].get()))
                for e in extras:
                    for line in e.log_lines(iteration, seen):
                        status(line)
                torch.cuda.reset_peak_memory_stats()
            if writer and params.save_example_period > 0 and ((iteration == 1 and params.save_initial_examples) or
                                                              iteration % params.save_example_period == 0):
                from .samples import save_frames, save_sentences
                status('saving to %s (iteration %d)' % (params.out_samples, iteration))
                save_frames(xs[0], '%s/real_samples.png' % params.out_samples)
                if gan.gen_ema is not None:
                    step = graphed.ts if use_graph else ts
                    fake = _averaged_samples(gan, step._z, None if step.conds is None else step.conds[0])
                    status('fake samples of iteration %d come from the averaged generator (%d updates)' % (iteration,
                                                                                                        gan.gen_ema.updates))
                for f in fake:
                    h, w = f.size(3), f.size(4)
                    save_frames(f.detach(), '%s/fake_samples_epoch_%03d_iter_%06d_%dx%d.png' % (params.out_samples, epoch,
                                                                                                 iteration, h, w))
                if cond is not None and vocab is not None:
                    save_sentences(y[0], path='%s/sentences_epoch%03d_iter_%06d.txt' % (params.out_samples, epoch, iteration),
                                   vocab=vocab)
            if kid is not None:
                kid.step(iteration)              # evaluates, logs and appends to <out>/metrics.jsonl when one is due
            load_watch.start()
            iter_watch.stop()
            avg_iter.update(iter_watch.elapsed_time)
            iter_watch.start()
            x, y = pre.next()
            i += 1
            if max_iters is not None and iteration >= max_iters:
                return iteration
    return iteration
